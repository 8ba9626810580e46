// Multilayer perceptron classifier on gfx950 / MI355X: the fused forward / backward pass and the forward row pass of
// models/classification/mlp.py MlpObjFunc and MlpcModelMapper (ops/mlp_fused.py), for contiguous fp64 rows X [n, d0],
// layers = [d0, h.., C] with 1 to 3 affine layers (0, 1 or 2 hidden sigmoid layers, a softmax + cross-entropy top),
// fp64 class indices y in [0, C) and weights w.  All arithmetic is fp64; no [n, width] block of activations or deltas
// is ever written to memory.
//
// Compile-time shape.  Tile counts (tiles of 16) are template parameters so that every accumulator index is static,
// rounded up to bound the instantiations: input tiles TI = 1, 2, 4 or 8 (gradient pass), class tiles TO = 1, 2 or 4,
// and one common count TH = 1, 2 or 4 for both hidden layers.  The extra tiles are zero padding in the images (a
// padded hidden unit has activation 0.5 and meets zero weights in the next layer and in the transposed image, so it
// contributes exactly 0 everywhere; its Gram rows and columns are not stored).
//
// The weight pack (ops/mlp_fused.weight_pack), per layer l with KT = in tiles and NT = out tiles, in this order:
//   fwd  [NT][KT][g = 4][mm = 16][s = 4], element = W_l[16 kt + 4 g + s, 16 nt + mm]      (W_l is [in, out])
//   bias [16 NT]
//   bwd  [KT][NT][g][mm][s],              element = W_l[16 kt + mm, 16 nt + 4 g + s]      (gradient pass, l >= 1 only)
// fwd and bwd are the same builder applied to W_l and to its transpose.  All images are read through the caches, not
// staged in LDS: the batch's activations take the LDS (below), and the gradient pass's pack is at most 130 KiB
// (TI TH TO = 4 4 2 with two hidden layers), resident in L2; a weight set of the row pass is under 600 KiB (d0 = 1024).
//
// MFMA maps (dense64_mfma.h): the image is the A operand (row mm = output 16 nt + mm, k = g), the data rows are the B
// operand (k = g, column mm = the lane's data row); lane (mm, g) holds outputs 16 nt + g + 4 q of its row mm.
//
// alink_mlp_fused_grad_f64 (d0 <= 128, hidden <= 64, C <= 64): one read of X gives [sum w loss | flat gradient in the
// coef layout].  A workgroup of 4 waves owns a row chunk and walks it 64 rows at a time; a wave owns 16 rows through
// the forward and backward pass:
//   forward   layer 0 from the row's dims in registers (load_group), accumulators started at the bias; the sigmoid is
//             1.0 / (1.0 + exp(-z)) as bias_sigmoid_kernel; S_l goes to LDS from the registers that hold it and the
//             next layer reads dims 4 g + s of row mm back as its B operand after a wave-level LDS wait (a wave needs
//             only its own rows).
//   top       no pivot class (ops/softmax.softmax_full_grad_torch): the maximum over the lane's own accumulators, then
//             group_max; the exp terms in ascending class order per lane, then group_sum; lse = mx + log(se),
//             loss = lse - z[y], D_L = w (exp(z - lse) - [c == y]).  A padded class slot gives exactly 0 and never
//             enters the maximum.
//   backward  per layer from the top, after a workgroup barrier: dW_l += H_l^T D_{l+1} on MFMA, four rows per
//             instruction (A[mm][g] = H_l[i0 + g][16 ta + mm], B[g][mm] = D_{l+1}[i0 + g][16 tb + mm], slot q =
//             dW_l[16 ta + g + 4 q][16 tb + mm]); the tiles of all layers form one list (layer, ta, tb ascending) and
//             tile t belongs to wave t mod 4, accumulator t / 4 (at most 10 per wave), kept in registers for the whole
//             chunk; a list shorter than 4 tiles is held by every wave for its own 16 rows and the waves are added
//             through LDS in wave order at the chunk's end (the rules of WaveDeal in gram64_mfma.h, written out here:
//             its finish, with the store dispatched per wave, measured 46 % slower in this kernel,
//             profiles/ordered_sum.txt).  db_l: thread (wave, lane) adds column `lane` of D_{l+1} over the wave's 16
//             rows in row order, batch after batch; the four waves are added in wave order at the chunk's end.
//             D_l = (D_{l+1} W_l^T) * S_l (1 - S_l) on MFMA against the bwd image, each wave for its own rows, and
//             written over S_l once a second barrier says every wave's Gram reads of S_l are done.
//   merge     part [nchunk, 1 + nw], merged in chunk order (ordered_sum.h): the same bits for every grid and run.
// LDS plan of the gradient pass (bytes; rows 16 T doubles apart, columns xor-ed with 16 on odd rows when T is even, so
// that rows of either parity start 32 banks apart):
//   xs  X batch         64 x 16 TI x 8   =  8 / 16 / 32 / 64 KiB
//   sb  S_l, then D_l   (L - 1) x 64 x 16 TH x 8 = 0 .. 64 KiB
//   da  D_L             64 x 16 TO x 8   =  8 / 16 / 32 KiB
//   red split-rule sums 4 NTILES x 2 KiB (NTILES < 4 only), dbr 4 x 64 x 8 per layer, wl 32 bytes.
// Tile budget: the rounded tile counts of all layers add to at most ML_MAX_TILES = 40, that is 10 accumulator tiles per
// wave.  The design target was 64; the instantiations with 48 and more tiles (TI TH TO = 8 4 4 with one hidden layer;
// 4 4 4, 8 4 1, 8 4 2 and 8 4 4 with two) spill to scratch (148 .. 668 bytes per lane), and the last does not fit the
// 160 KiB of LDS either, so those shape classes are refused here and stay on the GEMM path (ops/mlp.py).  Every
// instantiation that is left uses no scratch (profiles/mlp_fused.txt).
//
// alink_mlp_fused_rows_f64 (d0 <= 1024): the forward pass alone for S <= 8 weight sets.  Layer 0 walks the dims in
// tiles of 16 for groups of 8 / T1 sets at once (T1 = out tiles of layer 0; 8 accumulator tiles), so X is read from
// memory once and again from the caches for a further group; the group's first-layer outputs go to LDS (64 KiB), and
// the rest of the network runs set by set from there.  Outputs by mask: 1 sums [S] = sum w (lse - z[y]) (one partial
// per 64-row batch and set, part [S, nb], added per set by the batch sums of ordered_sum.h: independent of the
// grid); for S = 1: 2 row_loss [n] = min(lse - z[y], -log(1e-300)) (the clamp of -log(max(P[y], 1e-300))), 4 P [n, C]
// = exp(z - mx) / se, 8 label [n] (int32) = the first maximum of the logits (own accumulators in ascending class
// order first, the four lane groups last, the lower class on equal bits; never a padded slot).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "dense64_mfma.h"
#include "ordered_sum.h"

#pragma clang fp contract(off)

namespace {

using namespace d64;

constexpr int ML_MAX_IN = 128, ML_MAX_HIDDEN = 64, ML_MAX_CLASSES = 64, ML_ROWS_MAX_IN = 1024, ML_MAX_STEPS = 8;
constexpr int ML_LDS = 160 * 1024 - 512;    // what a workgroup may take
constexpr int ML_MAX_TILES = 40;            // Gram tiles of all layers: more spill to scratch
enum { M_LOSS = 1, M_ROW_LOSS = 2, M_P = 4, M_LABEL = 8 };

struct Dims {
    int d[4];       // layers, d[nl] = C
};

// offsets (doubles) into one weight set of the pack
struct Pack {
    int fwd[3], bias[3], bwd[3], size;
};

constexpr Pack make_pack(int nl, int ti, int th, int to, bool with_bwd) {
    Pack p{};
    int o = 0;
    for (int l = 0; l < nl; ++l) {
        const int a = l == 0 ? ti : th, b = l == nl - 1 ? to : th;
        p.fwd[l] = o;
        o += a * b * 256;
        p.bias[l] = o;
        o += 16 * b;
        p.bwd[l] = o;
        if (with_bwd && l > 0) o += a * b * 256;
    }
    p.size = o;
    return p;
}

constexpr int l_tin(int ti, int th, int l) { return l == 0 ? ti : th; }
constexpr int l_tout(int nl, int th, int to, int l) { return l == nl - 1 ? to : th; }
constexpr int l_toff(int nl, int ti, int th, int to, int l) {
    int o = 0;
    for (int i = 0; i < l; ++i) o += l_tin(ti, th, i) * l_tout(nl, th, to, i);
    return o;
}

__device__ __forceinline__ int coef_off(const Dims& dm, int l) {
    int o = 0;
    for (int i = 0; i < l; ++i) o += dm.d[i] * dm.d[i + 1] + dm.d[i + 1];
    return o;
}

// LDS writes of this wave's lanes become visible to its other lanes: the wave's DS operations complete in order, so
// no workgroup barrier is needed for rows that only this wave touches
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// element (row, col) of a [64, 16 T] LDS block
template <int T>
__device__ __forceinline__ int sidx(int row, int col) {
    return row * (16 * T) + (T % 2 == 0 ? col ^ ((row & 1) << 4) : col);
}

template <int T>
__device__ __forceinline__ void init_bias(d4_t (&e)[T], const double* __restrict__ bias, int g) {
#pragma unroll
    for (int t = 0; t < T; ++t) {
#pragma unroll
        for (int q = 0; q < 4; ++q) e[t][q] = bias[16 * t + g + 4 * q];
    }
}

// one k tile of a product: e[t] += image tile (t, tk) . b, b = the lane's row at dims 16 tk + 4 g + s
template <int TN>
__device__ __forceinline__ void affine_tile(d4_t (&e)[TN], const double* __restrict__ img, int ktiles, int tk, int g,
                                            int mm, d4_t b) {
    d4_t a[TN];
#pragma unroll
    for (int t = 0; t < TN; ++t)
        a[t] = *reinterpret_cast<const d4_t*>(img + (((t * ktiles + tk) * 4 + g) * 16 + mm) * 4);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
#pragma unroll
        for (int t = 0; t < TN; ++t) e[t] = mf64(a[t][s], b[s], e[t]);
    }
}

// e[t] += sum_k in[lr][k] M[k][16 t + ..] with the lane's row read from the LDS block `in` [64, 16 TK]
template <int TK, int TN>
__device__ __forceinline__ void affine_lds(d4_t (&e)[TN], const double* __restrict__ img, const double* in, int lr,
                                           int g, int mm) {
#pragma unroll
    for (int tk = 0; tk < TK; ++tk)
        affine_tile<TN>(e, img, TK, tk, g, mm, *reinterpret_cast<const d4_t*>(in + sidx<TK>(lr, 16 * tk + 4 * g)));
}

// out[lr][16 t + g + 4 q] = sigmoid(e[t][q])
template <int T>
__device__ __forceinline__ void sigmoid_store(const d4_t (&e)[T], double* out, int lr, int g) {
#pragma unroll
    for (int t = 0; t < T; ++t) {
#pragma unroll
        for (int q = 0; q < 4; ++q) out[sidx<T>(lr, 16 * t + g + 4 * q)] = 1.0 / (1.0 + exp(-e[t][q]));
    }
}

// the row's maximum logit and sum of exp(z - mx) over the classes < C; the four lanes of a row return the same bits
template <int T>
__device__ __forceinline__ void top_sums(const d4_t (&z)[T], int C, int g, double& mx, double& se) {
    mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < T; ++t) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (16 * t + g + 4 * q < C) mx = fmax(mx, z[t][q]);
    }
    mx = group_max(mx);
    se = 0.0;
#pragma unroll
    for (int t = 0; t < T; ++t) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (16 * t + g + 4 * q < C) se += exp(z[t][q] - mx);
    }
    se = group_sum(se);
}

// The layout and the tile deal of the gradient pass.
template <int NL, int TI, int TH, int TO>
struct Net {
    static constexpr int NH = NL - 1;
    static constexpr int NTILES = l_toff(NL, TI, TH, TO, NL);
    static constexpr bool SPLIT = NTILES < 4;                   // the waves split the rows, not the tiles
    static constexpr int MAXT = SPLIT ? NTILES : (NTILES + 3) / 4;
    static constexpr int RED = SPLIT ? 4 * NTILES * 256 : 4;
    static constexpr int LDS_BYTES = 8 * (1024 * TI + NH * 1024 * TH + 1024 * TO + RED + NL * 256 + 4);
    static constexpr bool FITS = LDS_BYTES <= ML_LDS && NTILES <= ML_MAX_TILES;
    static constexpr int tin(int l) { return l_tin(TI, TH, l); }
    static constexpr int tout(int l) { return l_tout(NL, TH, TO, l); }
    static constexpr int toff(int l) { return l_toff(NL, TI, TH, TO, l); }
    static constexpr Pack pack() { return make_pack(NL, TI, TH, TO, true); }

    // dW_L += H_L^T D_{L+1} over the staged batch, and the lane's column of db_L
    template <int L>
    static __device__ __forceinline__ void gram(d4_t (&acc)[MAXT], double& db, const double* hs, const double* ds,
                                                int wave, int lane) {
        constexpr int TA = tin(L), TB = tout(L), T0 = toff(L);
        const int mm = lane & 15, g = lane >> 4;
        const int base = SPLIT ? 16 * wave : 0;
#pragma unroll
        for (int s = 0; s < MAXT; ++s) {
            const int tt = (SPLIT ? s : wave + 4 * s) - T0;     // wave-uniform
            if (tt < 0 || tt >= TA * TB) continue;
            const int ca = 16 * (tt / TB) + mm, cb = 16 * (tt % TB) + mm;
            d4_t a = acc[s];
#pragma unroll 4
            for (int r4 = 0; r4 < (SPLIT ? 4 : 16); ++r4) {
                const int row = base + 4 * r4 + g;
                a = mf64(hs[sidx<TA>(row, ca)], ds[sidx<TB>(row, cb)], a);
            }
            acc[s] = a;
        }
        if (lane < 16 * TB) {
#pragma unroll 4
            for (int r = 0; r < 16; ++r) db += ds[sidx<TB>(16 * wave + r, lane)];
        }
    }

    // the layers L .. 0 of the backward pass of one batch; every thread of the workgroup calls it
    template <int L>
    static __device__ __forceinline__ void backward(d4_t (&acc)[MAXT], double (&db)[NL], double* xs,
                                                    double (*sb)[NH > 0 ? 1024 * TH : 4], double* da,
                                                    const double* __restrict__ pk, int wave, int lane, int lr) {
        const double* hs = L == 0 ? xs : sb[L > 0 ? L - 1 : 0];
        const double* ds = L == NL - 1 ? da : sb[L < NH ? L : 0];
        __syncthreads();        // H_L and D_{L+1} of all 64 rows are staged
        gram<L>(acc, db[L], hs, ds, wave, lane);
        if constexpr (L > 0) {
            constexpr int TB = tout(L);
            const int mm = lane & 15, g = lane >> 4;
            double* sl = sb[L - 1];
            d4_t dl[TH];
#pragma unroll
            for (int t = 0; t < TH; ++t) dl[t] = d4_t{0.0, 0.0, 0.0, 0.0};
            affine_lds<TB, TH>(dl, pk + pack().bwd[L], ds, lr, g, mm);
#pragma unroll
            for (int t = 0; t < TH; ++t) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const double s = sl[sidx<TH>(lr, 16 * t + g + 4 * q)];
                    dl[t][q] = dl[t][q] * (s * (1.0 - s));
                }
            }
            __syncthreads();    // every wave's Gram reads of S_L are done: D_L takes its place
#pragma unroll
            for (int t = 0; t < TH; ++t) {
#pragma unroll
                for (int q = 0; q < 4; ++q) sl[sidx<TH>(lr, 16 * t + g + 4 * q)] = dl[t][q];
            }
            backward<L - 1>(acc, db, xs, sb, da, pk, wave, lane, lr);
        }
    }

    // slot s of a lane -> the chunk's partial pc = [loss | coef layout]
    static __device__ __forceinline__ void store(const d4_t (&acc)[MAXT], double* __restrict__ pc, const Dims& dm,
                                                 int wave, int lane) {
        const int mm = lane & 15, g = lane >> 4;
#pragma unroll
        for (int s = 0; s < MAXT; ++s) {
            const int t = SPLIT ? s : wave + 4 * s;
#pragma unroll
            for (int l = 0; l < NL; ++l) {
                const int tt = t - toff(l);
                if (tt < 0 || tt >= tin(l) * tout(l)) continue;
                const int out = 16 * (tt % tout(l)) + mm, off = 1 + coef_off(dm, l);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int in = 16 * (tt / tout(l)) + g + 4 * q;
                    if (in < dm.d[l] && out < dm.d[l + 1]) pc[off + in * dm.d[l + 1] + out] = acc[s][q];
                }
            }
        }
    }
};

template <int NL, int TI, int TH, int TO>
__global__ __launch_bounds__(256) void mlp_grad_kernel(
        const double* __restrict__ X, const double* __restrict__ y, const double* __restrict__ w, int64_t n, Dims dm,
        const double* __restrict__ pack, int vec, int64_t chunk_rows, int64_t nchunk, int64_t P,
        double* __restrict__ part) {
    using N = Net<NL, TI, TH, TO>;
    constexpr int NH = N::NH;
    constexpr Pack PK = N::pack();
    __shared__ __attribute__((aligned(32))) double xs[1024 * TI];
    __shared__ __attribute__((aligned(32))) double sb[NH > 0 ? NH : 1][NH > 0 ? 1024 * TH : 4];
    __shared__ __attribute__((aligned(32))) double da[1024 * TO];
    __shared__ __attribute__((aligned(32))) double red[N::RED];
    __shared__ double dbr[NL][4][64];
    __shared__ double wl[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int mm = lane & 15, g = lane >> 4;
    const int lr = wave * 16 + mm;          // the lane's row of a batch
    const int d0 = dm.d[0], C = dm.d[NL];
    for (int64_t c = blockIdx.x; c < nchunk; c += gridDim.x) {
        const int64_t r0 = c * chunk_rows;
        const int64_t r1 = r0 + chunk_rows < n ? r0 + chunk_rows : n;
        d4_t acc[N::MAXT];
#pragma unroll
        for (int s = 0; s < N::MAXT; ++s) acc[s] = d4_t{0.0, 0.0, 0.0, 0.0};
        double db[NL];
#pragma unroll
        for (int l = 0; l < NL; ++l) db[l] = 0.0;
        double lsum = 0.0;
        for (int64_t bb = r0; bb < r1; bb += 64) {
            const int64_t i = bb + lr;
            const bool ok = i < r1;
            const double* __restrict__ xr = X + (ok ? i : r0) * (int64_t)d0;
            const double wi = ok ? w[i] : 0.0;
            const int yi = ok ? (int)y[i] : C;
            // The pack does not change from batch to batch; its reads are tied to a zero the compiler cannot see
            // through, or they would be hoisted out of the batch loop into registers and spill.
            int pin = 0;
            asm volatile("" : "+v"(pin));
            const double* __restrict__ pk = pack + pin;
            d4_t z[TO];
            {
                d4_t xb[TI];
#pragma unroll
                for (int ti = 0; ti < TI; ++ti) {
                    xb[ti] = vec ? load_group<true>(xr, ok, 16 * ti + 4 * g, d0)
                                 : load_group<false>(xr, ok, 16 * ti + 4 * g, d0);
                    *reinterpret_cast<d4_t*>(xs + sidx<TI>(lr, 16 * ti + 4 * g)) = xb[ti];
                }
                if constexpr (NL == 1) {
                    init_bias<TO>(z, pk + PK.bias[0], g);
#pragma unroll
                    for (int ti = 0; ti < TI; ++ti) affine_tile<TO>(z, pk + PK.fwd[0], TI, ti, g, mm, xb[ti]);
                } else {
                    d4_t h[TH];
                    init_bias<TH>(h, pk + PK.bias[0], g);
#pragma unroll
                    for (int ti = 0; ti < TI; ++ti) affine_tile<TH>(h, pk + PK.fwd[0], TI, ti, g, mm, xb[ti]);
                    sigmoid_store<TH>(h, sb[0], lr, g);
                    wave_lds_sync();
                }
            }
            if constexpr (NL == 3) {
                d4_t h[TH];
                init_bias<TH>(h, pk + PK.bias[1], g);
                affine_lds<TH, TH>(h, pk + PK.fwd[1], sb[0], lr, g, mm);
                sigmoid_store<TH>(h, sb[1], lr, g);
                wave_lds_sync();
            }
            if constexpr (NL > 1) {
                init_bias<TO>(z, pk + PK.bias[NL - 1], g);
                affine_lds<TH, TO>(z, pk + PK.fwd[NL - 1], sb[NH > 0 ? NH - 1 : 0], lr, g, mm);
            }
            double mx, se;
            top_sums<TO>(z, C, g, mx, se);
            const double lse = mx + log(se);
            double zy = 0.0;
#pragma unroll
            for (int t = 0; t < TO; ++t) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int cls = 16 * t + g + 4 * q;
                    double r = 0.0;
                    if (cls < C) {
                        r = exp(z[t][q] - lse);
                        if (cls == yi) {
                            r -= 1.0;
                            zy = z[t][q];
                        }
                        r *= wi;
                    }
                    da[sidx<TO>(lr, cls)] = r;
                }
            }
            zy = group_sum(zy);
            if (g == 0) lsum += (lse - zy) * wi;
            N::template backward<NL - 1>(acc, db, xs, sb, da, pk, wave, lane, lr);
            __syncthreads();        // the batch's reads are done before the next one is staged
        }
        double* __restrict__ pc = part + c * P;
        lsum = osum::wave_sum_asc(lsum);    // the lanes with g > 0 add zeros
        if (lane == 0) wl[wave] = lsum;
#pragma unroll
        for (int l = 0; l < NL; ++l) dbr[l][wave][lane] = db[l];
        if constexpr (N::SPLIT) {
#pragma unroll
            for (int s = 0; s < N::MAXT; ++s)
                *reinterpret_cast<d4_t*>(red + ((wave * N::NTILES + s) * 64 + lane) * 4) = acc[s];
        }
        __syncthreads();
        if (tid == 0) pc[0] = ((wl[0] + wl[1]) + wl[2]) + wl[3];
        if (wave == 0) {
#pragma unroll
            for (int l = 0; l < NL; ++l)
                if (lane < dm.d[l + 1])
                    pc[1 + coef_off(dm, l) + dm.d[l] * dm.d[l + 1] + lane] =
                        ((dbr[l][0][lane] + dbr[l][1][lane]) + dbr[l][2][lane]) + dbr[l][3][lane];
        }
        if constexpr (N::SPLIT) {
            if (wave == 0) {
#pragma unroll
                for (int s = 0; s < N::MAXT; ++s) {
                    d4_t a = *reinterpret_cast<const d4_t*>(red + (s * 64 + lane) * 4);
                    for (int ws = 1; ws < 4; ++ws)
                        a += *reinterpret_cast<const d4_t*>(red + ((ws * N::NTILES + s) * 64 + lane) * 4);
                    acc[s] = a;
                }
                N::store(acc, pc, dm, wave, lane);
            }
        } else {
            N::store(acc, pc, dm, wave, lane);
        }
        __syncthreads();            // wl, dbr and red may be written again
    }
}

template <int NL, int TH, int TO, bool VEC>
__global__ __launch_bounds__(256) void mlp_rows_kernel(
        const double* __restrict__ X, const double* __restrict__ y, const double* __restrict__ w, int64_t n, Dims dm,
        const double* __restrict__ pack, int nti, int S, int mask, double* __restrict__ part, int64_t nb,
        double* __restrict__ row_loss, double* __restrict__ Pout, int* __restrict__ label) {
    constexpr int T1 = NL == 1 ? TO : TH;       // out tiles of layer 0
    constexpr int SG = 8 / T1;                  // weight sets per walk of the dims
    __shared__ __attribute__((aligned(32))) double s1[SG][1024 * T1];
    __shared__ __attribute__((aligned(32))) double s2[NL == 3 ? 1024 * TH : 4];
    __shared__ double ws[ML_MAX_STEPS][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mm = lane & 15, g = lane >> 4;
    const int lr = wave * 16 + mm;
    const int d0 = dm.d[0], C = dm.d[NL];
    const Pack pk = make_pack(NL, nti, TH, TO, false);
    for (int64_t b = blockIdx.x; b < nb; b += gridDim.x) {
        const int64_t row = b * ROWS + lr;
        const bool ok = row < n;
        const double* __restrict__ xr = X + (ok ? row : 0) * (int64_t)d0;
        const double wi = ok ? w[row] : 0.0;
        const int yi = ok ? (int)y[row] : C;
        for (int s0 = 0; s0 < S; s0 += SG) {
            {
                d4_t e[SG][T1];
                const double* __restrict__ pj[SG];
#pragma unroll
                for (int j = 0; j < SG; ++j) {      // a set past the last repeats it; its result is not used
                    pj[j] = pack + (int64_t)(s0 + j < S ? s0 + j : S - 1) * pk.size;
                    init_bias<T1>(e[j], pj[j] + pk.bias[0], g);
                }
                for (int ti = 0; ti < nti; ++ti) {
                    const d4_t xg = load_group<VEC>(xr, ok, 16 * ti + 4 * g, d0);
#pragma unroll
                    for (int j = 0; j < SG; ++j) affine_tile<T1>(e[j], pj[j] + pk.fwd[0], nti, ti, g, mm, xg);
                }
#pragma unroll
                for (int j = 0; j < SG; ++j) {
                    if constexpr (NL > 1) {
                        sigmoid_store<T1>(e[j], s1[j], lr, g);
                    } else {
#pragma unroll
                        for (int t = 0; t < T1; ++t) {
#pragma unroll
                            for (int q = 0; q < 4; ++q) s1[j][sidx<T1>(lr, 16 * t + g + 4 * q)] = e[j][t][q];
                        }
                    }
                }
            }
            wave_lds_sync();
            const int nj = S - s0 < SG ? S - s0 : SG;
            for (int j = 0; j < nj; ++j) {
                const double* __restrict__ pw = pack + (int64_t)(s0 + j) * pk.size;
                d4_t z[TO];
                if constexpr (NL == 1) {
#pragma unroll
                    for (int t = 0; t < TO; ++t) {
#pragma unroll
                        for (int q = 0; q < 4; ++q) z[t][q] = s1[j][sidx<TO>(lr, 16 * t + g + 4 * q)];
                    }
                } else if constexpr (NL == 2) {
                    init_bias<TO>(z, pw + pk.bias[1], g);
                    affine_lds<TH, TO>(z, pw + pk.fwd[1], s1[j], lr, g, mm);
                } else {
                    d4_t h[TH];
                    init_bias<TH>(h, pw + pk.bias[1], g);
                    affine_lds<TH, TH>(h, pw + pk.fwd[1], s1[j], lr, g, mm);
                    sigmoid_store<TH>(h, s2, lr, g);
                    wave_lds_sync();
                    init_bias<TO>(z, pw + pk.bias[2], g);
                    affine_lds<TH, TO>(z, pw + pk.fwd[2], s2, lr, g, mm);
                }
                double mx, se;
                top_sums<TO>(z, C, g, mx, se);
                const double lse = mx + log(se);
                double zy = 0.0, bv = -INFINITY;
                int bi = 0x7fffffff;
#pragma unroll
                for (int t = 0; t < TO; ++t) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int cls = 16 * t + g + 4 * q;
                        if (cls < C) {
                            if (cls == yi) zy = z[t][q];
                            if (z[t][q] > bv) {
                                bv = z[t][q];
                                bi = cls;
                            }
                            if ((mask & M_P) && ok) Pout[row * C + cls] = exp(z[t][q] - mx) / se;
                        }
                    }
                }
                zy = group_sum(zy);
                if (mask & M_LOSS) {
                    const double v = osum::wave_sum_asc(g == 0 ? (lse - zy) * wi : 0.0);
                    if (lane == 0) ws[s0 + j][wave] = v;
                }
                if ((mask & M_ROW_LOSS) && ok && g == 0) row_loss[row] = fmin(lse - zy, -log(1e-300));
                if (mask & M_LABEL) {
#pragma unroll
                    for (int o = 16; o < 64; o <<= 1) {
                        const double ov = __shfl_xor(bv, o, 64);
                        const int oi = __shfl_xor(bi, o, 64);
                        if (ov > bv || (ov == bv && oi < bi)) {
                            bv = ov;
                            bi = oi;
                        }
                    }
                    if (ok && g == 0) label[row] = bi < C ? bi : 0;
                }
                wave_lds_sync();        // the reads of s2 are done before the next set writes it
            }
        }
        if (mask & M_LOSS) {
            __syncthreads();
            if (tid < S) part[(int64_t)tid * nb + b] = ((ws[tid][0] + ws[tid][1]) + ws[tid][2]) + ws[tid][3];
            __syncthreads();        // ws may be written again
        }
    }
}

template <int NL, int TI, int TH, class... A>
bool grad_to(int to, unsigned blocks, hipStream_t st, A... a) {
#define ALINK_ML_GRAD(TO)                                                                                          \
    if constexpr (Net<NL, TI, TH, TO>::FITS) {                                                                   \
        hipLaunchKernelGGL((mlp_grad_kernel<NL, TI, TH, TO>), dim3(blocks), dim3(256), 0, st, a...);               \
        return true;                                                                                               \
    } else {                                                                                                       \
        return false;                                                                                              \
    }
    if (to == 1) { ALINK_ML_GRAD(1) }
    if (to == 2) { ALINK_ML_GRAD(2) }
    ALINK_ML_GRAD(4)
#undef ALINK_ML_GRAD
}

template <int NL, int TI, class... A>
bool grad_th(int th, int to, unsigned blocks, hipStream_t st, A... a) {
    if constexpr (NL == 1) {
        return grad_to<NL, TI, 1>(to, blocks, st, a...);
    } else {
        if (th == 1) return grad_to<NL, TI, 1>(to, blocks, st, a...);
        if (th == 2) return grad_to<NL, TI, 2>(to, blocks, st, a...);
        return grad_to<NL, TI, 4>(to, blocks, st, a...);
    }
}

template <int NL, class... A>
bool grad_ti(int ti, int th, int to, unsigned blocks, hipStream_t st, A... a) {
    if (ti == 1) return grad_th<NL, 1>(th, to, blocks, st, a...);
    if (ti == 2) return grad_th<NL, 2>(th, to, blocks, st, a...);
    if (ti == 4) return grad_th<NL, 4>(th, to, blocks, st, a...);
    return grad_th<NL, 8>(th, to, blocks, st, a...);
}

template <int NL, int TH, class... A>
void rows_to(int to, bool vec, unsigned blocks, hipStream_t st, A... a) {
#define ALINK_ML_ROWS(TO)                                                                                          \
    do {                                                                                                           \
        if (vec) hipLaunchKernelGGL((mlp_rows_kernel<NL, TH, TO, true>), dim3(blocks), dim3(256), 0, st, a...);    \
        else hipLaunchKernelGGL((mlp_rows_kernel<NL, TH, TO, false>), dim3(blocks), dim3(256), 0, st, a...);       \
    } while (0)
    if (to == 1) ALINK_ML_ROWS(1);
    else if (to == 2) ALINK_ML_ROWS(2);
    else ALINK_ML_ROWS(4);
#undef ALINK_ML_ROWS
}

template <int NL, class... A>
void rows_th(int th, int to, bool vec, unsigned blocks, hipStream_t st, A... a) {
    if constexpr (NL == 1) {
        rows_to<NL, 1>(to, vec, blocks, st, a...);
    } else {
        if (th == 1) rows_to<NL, 1>(to, vec, blocks, st, a...);
        else if (th == 2) rows_to<NL, 2>(to, vec, blocks, st, a...);
        else rows_to<NL, 4>(to, vec, blocks, st, a...);
    }
}

inline int round_tiles(int d, int cap) {       // ceil(d / 16) rounded up to 1, 2, 4 (or 8)
    const int t = (d + 15) / 16;
    int r = 1;
    while (r < t) r *= 2;
    return r <= cap ? r : 0;
}

// the checks both entry points share: 0 when the layers are in range, with the rounded hidden and class tile counts
inline int check_layers(int nl, const Dims& dm, int max_in, int* th, int* to) {
    if (nl < 1 || nl > 3 || dm.d[0] < 1 || dm.d[0] > max_in || dm.d[nl] < 2 || dm.d[nl] > ML_MAX_CLASSES) return 1;
    *th = 1;
    for (int l = 1; l < nl; ++l) {
        if (dm.d[l] < 1 || dm.d[l] > ML_MAX_HIDDEN) return 1;
        const int t = round_tiles(dm.d[l], 4);
        if (t > *th) *th = t;
    }
    *to = round_tiles(dm.d[nl], 4);
    return 0;
}

}  // namespace

extern "C" {

// One gradient pass over X [n, d0], y, w [n] of the network d0 -> d1 (-> d2 (-> d3)) with nl affine layers (unused
// widths are ignored), at the weights whose pack (fwd, bias, bwd per layer; tile counts rounded as the header says) is
// `pack`: out [1 + nw] = [sum w loss | gradient in the coef layout] through nchunk = ceil(n / chunk_rows) row chunks
// (chunk_rows a multiple of 64) whose partials part [nchunk, 1 + nw] are merged in chunk order.  Returns 1 for a
// shape outside the range, the classes over the tile budget included.
int alink_mlp_fused_grad_f64(const double* X, const double* y, const double* w, int64_t n, int nl, int d0, int d1,
                             int d2, int d3, const double* pack, int64_t chunk_rows, int64_t nchunk, double* part,
                             double* out, int grid, void* stream) {
    if (n <= 0) return 0;
    const Dims dm = {{d0, d1, d2, d3}};
    int th = 1, to = 1;
    if (n >= (1ll << 31) || check_layers(nl, dm, ML_MAX_IN, &th, &to)) return 1;
    if (chunk_rows < 64 || chunk_rows % 64 != 0 || nchunk != (n + chunk_rows - 1) / chunk_rows) return 1;
    if (X == nullptr || y == nullptr || w == nullptr || pack == nullptr || part == nullptr || out == nullptr) return 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int ti = round_tiles(d0, 8), vec = vec_ok(d0, X) ? 1 : 0;
    int64_t P = 1;
    for (int l = 0; l < nl; ++l) P += (int64_t)dm.d[l] * dm.d[l + 1] + dm.d[l + 1];
    const unsigned blocks = (unsigned)(grid > 0 && grid < nchunk ? grid : nchunk);
    bool ok;
    if (nl == 1) ok = grad_ti<1>(ti, th, to, blocks, st, X, y, w, n, dm, pack, vec, chunk_rows, nchunk, P, part);
    else if (nl == 2) ok = grad_ti<2>(ti, th, to, blocks, st, X, y, w, n, dm, pack, vec, chunk_rows, nchunk, P, part);
    else ok = grad_ti<3>(ti, th, to, blocks, st, X, y, w, n, dm, pack, vec, chunk_rows, nchunk, P, part);
    if (!ok) return 1;
    osum::chunk_merge(osum::Identity{}, P, nchunk, part, out, st);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

// The forward row pass over X [n, d0] (d0 <= 1024) for nsets <= 8 weight sets, pack [nsets][fwd, bias per layer] with
// ceil(d0 / 16) input tiles.  mask 1: out [nsets] = sum w loss per set, part [nsets, ceil(n / 64)]; with nsets = 1
// also mask 2: row_loss [n], 4: P [n, C], 8: label [n] (int32).
int alink_mlp_fused_rows_f64(const double* X, const double* y, const double* w, int64_t n, int nl, int d0, int d1,
                             int d2, int d3, const double* pack, int nsets, int mask, double* part, double* out,
                             double* row_loss, double* P, int* label, int grid, void* stream) {
    if (n <= 0) return 0;
    const Dims dm = {{d0, d1, d2, d3}};
    int th = 1, to = 1;
    if (n >= (1ll << 31) || check_layers(nl, dm, ML_ROWS_MAX_IN, &th, &to)) return 1;
    if (nsets < 1 || nsets > ML_MAX_STEPS || mask <= 0 || mask > 15 || (nsets > 1 && mask != M_LOSS)) return 1;
    if (X == nullptr || y == nullptr || w == nullptr || pack == nullptr) return 1;
    if ((mask & M_LOSS) && (part == nullptr || out == nullptr)) return 1;
    if (((mask & M_ROW_LOSS) && row_loss == nullptr) || ((mask & M_P) && P == nullptr) ||
        ((mask & M_LABEL) && label == nullptr))
        return 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int nti = (d0 + 15) / 16;
    const bool vec = vec_ok(d0, X);
    const int64_t nb = (n + ROWS - 1) / ROWS;
    const unsigned blocks = row_blocks(n, grid, 4096);
    if (nl == 1) rows_th<1>(th, to, vec, blocks, st, X, y, w, n, dm, pack, nti, nsets, mask, part, nb, row_loss, P, label);
    else if (nl == 2) rows_th<2>(th, to, vec, blocks, st, X, y, w, n, dm, pack, nti, nsets, mask, part, nb, row_loss, P, label);
    else rows_th<3>(th, to, vec, blocks, st, X, y, w, n, dm, pack, nti, nsets, mask, part, nb, row_loss, P, label);
    if (mask & M_LOSS) osum::batch_sums(part, nb, nsets, out, st);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // extern "C"
