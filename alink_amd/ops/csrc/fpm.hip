// Frequent-itemset support counting on vertical bitmaps (``ops/fpm.py``).  Bit t of row i of B [m, W] says that
// transaction t holds frequent item i; the support of an itemset is the popcount of the AND of its rows.  Every
// result is an integer sum of popcounts, so it is the same for every grid, chunk size and split of the words.
// Integer vector atomics only; the host oracle is ``models/associationrule/mining.fp_growth``.
//
// B is uint64 [m, W] with W even, so every row starts 16-byte aligned and two words move per load.  The bits past
// the last transaction and any padding word of a row are zero: the count kernels never mask.
//
// * alink_fpm_bitmap — the encoded transactions as CSR (crow int64 [n + 1], item int32 [nnz], ranks in [0, m),
//   unique within a row) into the zero-initialised B by a 32-bit OR per (transaction, item): a lane owns a
//   transaction, so the 64 lanes of a wave that hold one item OR into the same two dwords.  OR is order-free.  An
//   item outside [0, m) is skipped and counted in ``bad`` (the wrapper raises).
// * alink_fpm_pair_counts — the upper triangle of the bit Gram C[i][j] = popcount(B_i & B_j), i < j, uint32 [m, m].
//   A 256-thread workgroup owns a 64 x 64 block of item pairs (only blocks on or above the diagonal are launched)
//   and a range of the words.  It walks the range in chunks of KW words: both 64-row slabs of the chunk go through
//   registers into LDS word-major ([KW][64 + 2]), so a thread reads the 4 + 4 rows of its 4 x 4 pairs as two 32-byte
//   runs (a broadcast on the i side, 512 contiguous bytes per wave on the j side) and every word staged is used
//   64 times.  The 16 counters of a thread hold whole pairs: no cross-lane reduction, one add per (pair,
//   workgroup) at the end (a plain store when the workgroup owns all words).
// * alink_fpm_class_counts, alink_fpm_seq_counts — the walk (``fpm_walk_kernel``).  Candidates grouped by parent:
//   prefix int32 [classes, P], cls_ptr int64 [classes + 1] and ext int32 [candidates] as a CSR of each class's
//   extension codes; counts int64 [candidates].  A wave owns (class, range of ``chunk`` words) and takes the class's
//   extensions FPM_ET at a time: per step of 128 words it runs the parent's chain of P loads in two registers per
//   lane (``cur``), then per extension one 16-byte load, an AND and the word count into that extension's per-lane
//   counter.  The counters stay in registers across the steps of the range; a butterfly adds the lanes and lane 0
//   adds once per (candidate, unit).  A stateless policy, resolved at compile time, says what a code means:
//   - ``ItemsetStep`` (``ops/fpm.py``): a code is an item, every step is ``cur &= B[item]``, a word counts its set
//     bits.
//   - ``SeqStep<WB>`` (sequential patterns, ``ops/prefixspan.py``): B has one field of WB bits (8, 16, 32 or 64) per
//     sequence, 64 / WB sequences per word; bit j of sequence t's field in row i says that element j of the sequence
//     holds item i.  A code is 2 * item + s (s = 1: the item opens a new element, s = 0: it joins the last one), and
//     a pattern's bitmap holds bit j of a field when a match ends at element j: ``cur = B[item_0]``, S-step ``cur =
//     after(cur) & B[i]``, I-step ``cur &= B[i]``, where ``after`` keeps, in every field, the bits strictly above the
//     lowest set bit.  ``after(cur)`` is formed once per step and an extension ANDs with it or with ``cur`` by its
//     code's low bit; a word counts its non-zero fields.  The field masks are constants; no carry or shift leaves a
//     field.
//   Leaving out the extension loads of a step whose ``cur`` is zero in every lane was measured and dropped: it was no
//   faster (``profiles/fpgrowth.txt``).
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

typedef unsigned long long u64;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));

constexpr int FPM_THREADS = 256;
constexpr int FPM_TILE = 64;            // items per side of a pair block
constexpr int FPM_ET = 16;              // extensions of a class counted in one pass over the unit's words
constexpr int FPM_STEP = 128;           // words a wave covers per step (two per lane)

__global__ __launch_bounds__(FPM_THREADS) void fpm_bitmap_kernel(
        const int64_t* __restrict__ crow, const int* __restrict__ item, int64_t n, int m, int64_t W,
        uint32_t* __restrict__ B, int* __restrict__ bad) {
    for (int64_t t = (int64_t)blockIdx.x * FPM_THREADS + threadIdx.x; t < n; t += (int64_t)gridDim.x * FPM_THREADS) {
        const int64_t beg = crow[t], end = crow[t + 1];
        const int64_t dw = t >> 5;                          // little-endian: bit t of the uint64 row
        const uint32_t bit = 1u << (uint32_t)(t & 31);
        for (int64_t k = beg; k < end; ++k) {
            const int it = item[k];
            if (it < 0 || it >= m) {
                atomicAdd(bad, 1);
                continue;
            }
            atomicOr(B + ((int64_t)it * W * 2 + dw), bit);
        }
    }
}

// the upper-triangular block (bi <= bj) number ``b`` of a T x T block grid, row-major over the kept blocks
__device__ __forceinline__ void tri_block(int b, int T, int& bi, int& bj) {
    int i = 0, rowlen = T;
    while (b >= rowlen) {
        b -= rowlen;
        --rowlen;
        ++i;
    }
    bi = i;
    bj = i + b;
}

template <int KW>
__global__ __launch_bounds__(FPM_THREADS) void fpm_pair_kernel(
        const u64* __restrict__ B, int m, int64_t W, int T, int splits, int64_t words_per_split,
        uint32_t* __restrict__ C) {
    // two words of padding per LDS row: the staging writes of the 16 lanes that share a row of B spread over 8
    // banks instead of one, and every 4-row run stays 16-byte aligned
    __shared__ __attribute__((aligned(16))) u64 sa[KW][FPM_TILE + 2];
    __shared__ __attribute__((aligned(16))) u64 sb[KW][FPM_TILE + 2];
    const int blk = (int)(blockIdx.x / (unsigned)splits);
    const int sp = (int)(blockIdx.x % (unsigned)splits);
    int bi, bj;
    tri_block(blk, T, bi, bj);
    const int i0 = bi * FPM_TILE, j0 = bj * FPM_TILE;
    const int64_t w_lo = (int64_t)sp * words_per_split;
    const int64_t w_hi = w_lo + words_per_split < W ? w_lo + words_per_split : W;
    const int tid = threadIdx.x;
    const int ti = tid >> 4, tj = tid & 15;                 // the thread's 4 x 4 pairs: rows 4 ti.., columns 4 tj..
    uint32_t acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0;
    constexpr int PAIRS = KW / 2;                           // 16-byte pieces of a row's chunk
    for (int64_t w0 = w_lo; w0 < w_hi; w0 += KW) {
        // stage: piece p of row r, pieces fastest among the lanes (KW / 2 lanes read one row's 8 KW contiguous bytes)
        for (int e = tid; e < FPM_TILE * PAIRS; e += FPM_THREADS) {
            const int r = e / PAIRS, p = e % PAIRS;
            const int64_t w = w0 + 2 * p;                   // even, and W is even: w < w_hi covers w + 1
            u64x2 va = {0, 0}, vb = {0, 0};
            if (w < w_hi) {
                if (i0 + r < m) va = *reinterpret_cast<const u64x2*>(B + (int64_t)(i0 + r) * W + w);
                if (j0 + r < m) vb = *reinterpret_cast<const u64x2*>(B + (int64_t)(j0 + r) * W + w);
            }
            sa[2 * p][r] = va.x;
            sa[2 * p + 1][r] = va.y;
            sb[2 * p][r] = vb.x;
            sb[2 * p + 1][r] = vb.y;
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < KW; ++k) {
            const u64x2 a01 = *reinterpret_cast<const u64x2*>(&sa[k][4 * ti]);
            const u64x2 a23 = *reinterpret_cast<const u64x2*>(&sa[k][4 * ti + 2]);
            const u64x2 b01 = *reinterpret_cast<const u64x2*>(&sb[k][4 * tj]);
            const u64x2 b23 = *reinterpret_cast<const u64x2*>(&sb[k][4 * tj + 2]);
            const u64 a[4] = {a01.x, a01.y, a23.x, a23.y};
            const u64 b[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int y = 0; y < 4; ++y) acc[x][y] += (uint32_t)__popcll(a[x] & b[y]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        const int i = i0 + 4 * ti + x;
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            const int j = j0 + 4 * tj + y;
            if (i < j && j < m) {
                uint32_t* c = C + (int64_t)i * m + j;
                if (splits == 1) *c = acc[x][y];
                else if (acc[x][y]) atomicAdd(c, acc[x][y]);
            }
        }
    }
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += (uint32_t)__shfl_xor((int)v, s, 64);
    return v;
}

int fpm_cus() {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) return 256;
    return cus;
}

// the field constants of a w-bit layout: bit 0 of every field, and the in-field positions below s
template <int WB> struct Field {
    static constexpr u64 L = WB == 8 ? 0x0101010101010101ull : WB == 16 ? 0x0001000100010001ull
                             : WB == 32 ? 0x0000000100000001ull : 1ull;
    static constexpr u64 H = L << (WB - 1);
    static constexpr u64 low(int s) { return L * ((1ull << s) - 1ull); }
};

// in every field, the bits strictly above the lowest set bit (none when the field is zero or only its top bit is set)
template <int WB>
__device__ __forceinline__ u64 seq_after(u64 x) {
    if constexpr (WB == 64) {
        return x ? ~(x ^ (x - 1)) : 0ull;
    } else {
        u64 y = x;
#pragma unroll
        for (int s = 1; s <= WB / 2; s *= 2) y |= (y << s) & ~Field<WB>::low(s);     // smear upwards inside the field
        return (y << 1) & ~Field<WB>::L;
    }
}

// the number of non-zero fields: the add carries into a field's top bit when a lower bit is set, never beyond it
template <int WB>
__device__ __forceinline__ uint32_t seq_fields(u64 x) {
    constexpr u64 H = Field<WB>::H;
    return (uint32_t)__popcll((((x & ~H) + ~H) | x) & H);
}

// what a code of ``prefix`` / ``ext`` means to the walk: its row of B, whether the step first applies ``after``, and
// how a word of the result is counted
struct ItemsetStep {
    static __device__ __forceinline__ int row(int code) { return code; }
    static __device__ __forceinline__ bool shifts(int) { return false; }
    static __device__ __forceinline__ u64 after(u64 x) { return x; }
    static __device__ __forceinline__ uint32_t count(u64 x) { return (uint32_t)__popcll(x); }
};

template <int WB> struct SeqStep {
    static __device__ __forceinline__ int row(int code) { return code >> 1; }
    static __device__ __forceinline__ bool shifts(int code) { return code & 1; }
    static __device__ __forceinline__ u64 after(u64 x) { return seq_after<WB>(x); }
    static __device__ __forceinline__ uint32_t count(u64 x) { return seq_fields<WB>(x); }
};

template <class Step>
__global__ __launch_bounds__(FPM_THREADS) void fpm_walk_kernel(
        const u64* __restrict__ B, int64_t W, const int* __restrict__ prefix, int P,
        const int64_t* __restrict__ cls_ptr, const int* __restrict__ ext, int64_t n_classes,
        int64_t splits, int64_t chunk, u64* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (FPM_THREADS / 64) + (threadIdx.x >> 6);
    const int64_t nwave = (int64_t)gridDim.x * (FPM_THREADS / 64);
    const int64_t units = n_classes * splits;
    // every quantity that steers a loop or a branch below is the same in all 64 lanes of the wave
    for (int64_t u = wave; u < units; u += nwave) {
        const int64_t c = u / splits;
        const int64_t w_lo = (u - c * splits) * chunk;
        const int64_t w_hi = w_lo + chunk < W ? w_lo + chunk : W;
        const int64_t e_lo = cls_ptr[c], e_hi = cls_ptr[c + 1];
        const int* __restrict__ pre = prefix + c * P;
        for (int64_t e0 = e_lo; e0 < e_hi; e0 += FPM_ET) {
            const int ne = e_hi - e0 < FPM_ET ? (int)(e_hi - e0) : FPM_ET;
            uint32_t cnt[FPM_ET];
            const u64* rows[FPM_ET];
            bool sstep[FPM_ET];
#pragma unroll
            for (int e = 0; e < FPM_ET; ++e) {
                const int code = ext[e0 + (e < ne ? e : 0)];
                cnt[e] = 0;
                rows[e] = B + (int64_t)Step::row(code) * W;
                sstep[e] = Step::shifts(code);
            }
            for (int64_t w0 = w_lo; w0 < w_hi; w0 += FPM_STEP) {
                const int64_t w = w0 + 2 * lane;            // even, and W is even: w < w_hi covers w + 1
                const bool in = w < w_hi;
                u64x2 cur = {0, 0};
                if (in) {
                    cur = *reinterpret_cast<const u64x2*>(B + (int64_t)Step::row(pre[0]) * W + w);
                    for (int q = 1; q < P; ++q) {
                        const int code = pre[q];
                        const u64x2 v = *reinterpret_cast<const u64x2*>(B + (int64_t)Step::row(code) * W + w);
                        if (Step::shifts(code)) {
                            cur.x = Step::after(cur.x);
                            cur.y = Step::after(cur.y);
                        }
                        cur.x &= v.x;
                        cur.y &= v.y;
                    }
                }
                const u64x2 aft = {Step::after(cur.x), Step::after(cur.y)};
#pragma unroll
                for (int e = 0; e < FPM_ET; ++e) {
                    if (e < ne && in) {
                        const u64x2 v = *reinterpret_cast<const u64x2*>(rows[e] + w);
                        const u64x2 p = sstep[e] ? aft : cur;
                        cnt[e] += Step::count(v.x & p.x) + Step::count(v.y & p.y);
                    }
                }
            }
#pragma unroll
            for (int e = 0; e < FPM_ET; ++e) {
                if (e < ne) {
                    const uint32_t s = wave_sum(cnt[e]);
                    if (lane == 0 && s) atomicAdd(counts + e0 + e, (u64)s);
                }
            }
        }
    }
}

// the grid, the words per unit (a multiple of 128) and the units per class of the walk
void class_shape(int64_t W, int64_t n_classes, int grid, int64_t& chunk, int64_t& g, int64_t& splits) {
    g = grid > 0 ? grid : (int64_t)fpm_cus() * 16;
    const int64_t waves = g * (FPM_THREADS / 64);
    const int64_t steps = (W + FPM_STEP - 1) / FPM_STEP;
    if (chunk == 0) {
        int64_t s = (4 * waves + n_classes - 1) / n_classes;
        const int64_t most = (steps + 3) / 4;               // at least four steps per unit
        if (s > most) s = most;
        if (s < 1) s = 1;
        chunk = (steps + s - 1) / s * FPM_STEP;
    } else {
        chunk = (chunk + FPM_STEP - 1) / FPM_STEP * FPM_STEP;
    }
    splits = (W + chunk - 1) / chunk;
    if (grid <= 0 && n_classes * splits < waves) g = (n_classes * splits + 3) / 4;
}

template <class Step>
int launch_walk(const void* B, int64_t W, const int* prefix, int P, const int64_t* cls_ptr, const int* ext,
                int64_t n_classes, void* counts, int64_t chunk, int grid, hipStream_t stream) {
    if (W < 2 || (W & 1) || P < 1 || n_classes < 0 || chunk < 0) return 1;
    if (n_classes == 0) return 0;
    int64_t g, splits;
    class_shape(W, n_classes, grid, chunk, g, splits);
    hipLaunchKernelGGL(fpm_walk_kernel<Step>, dim3((unsigned)g), dim3(FPM_THREADS), 0, stream, (const u64*)B, W, prefix,
                       P, cls_ptr, ext, n_classes, splits, chunk, (u64*)counts);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // namespace

extern "C" {

// B must be zero on entry.  ``bad`` int32 [1], zero on entry, counts the items outside [0, m).
int alink_fpm_bitmap(const int64_t* crow, const int* item, int64_t n, int m, int64_t W, void* B, int* bad, int grid,
                     hipStream_t stream) {
    if (n < 0 || m < 1 || W < 2 || (W & 1) || W * 64 < n) return 1;
    if (n == 0) return 0;
    int64_t g = grid > 0 ? grid : (n + FPM_THREADS - 1) / FPM_THREADS;
    const int64_t cap = (int64_t)fpm_cus() * 16;
    if (grid <= 0 && g > cap) g = cap;
    hipLaunchKernelGGL(fpm_bitmap_kernel, dim3((unsigned)g), dim3(FPM_THREADS), 0, stream, crow, item, n, m, W,
                       (uint32_t*)B, bad);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

// C uint32 [m, m] must be zero on entry; only i < j is written.  ``chunk``: words staged per step, 16 or 32 (0: 32).
// ``splits``: workgroups that share the words of one block (0: enough to fill the chip).
int alink_fpm_pair_counts(const void* B, int m, int64_t W, void* C, int chunk, int splits, hipStream_t stream) {
    if (m < 1 || W < 2 || (W & 1)) return 1;
    if (chunk == 0) chunk = 32;
    if (chunk != 16 && chunk != 32) return 1;
    const int T = (m + FPM_TILE - 1) / FPM_TILE;
    const int64_t blocks = (int64_t)T * (T + 1) / 2;
    const int64_t steps = (W + chunk - 1) / chunk;
    int64_t s = splits;
    if (s <= 0) {
        s = ((int64_t)fpm_cus() * 32 + blocks - 1) / blocks;
        const int64_t most = (steps + 3) / 4;               // at least four steps per workgroup
        if (s > most) s = most;
    }
    if (s > steps) s = steps;
    if (s < 1) s = 1;
    const int64_t per = (steps + s - 1) / s * chunk;        // a multiple of the chunk: every range starts even
    s = (W + per - 1) / per;
    if (blocks * s > 0x7fffffffLL) return 1;
    const dim3 g((unsigned)(blocks * s));
    if (chunk == 16)
        hipLaunchKernelGGL(fpm_pair_kernel<16>, g, dim3(FPM_THREADS), 0, stream, (const u64*)B, m, W, T, (int)s, per,
                           (uint32_t*)C);
    else
        hipLaunchKernelGGL(fpm_pair_kernel<32>, g, dim3(FPM_THREADS), 0, stream, (const u64*)B, m, W, T, (int)s, per,
                           (uint32_t*)C);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

// counts int64 [candidates] must be zero on entry.  Items of ``prefix`` and ``ext_item`` lie in the rows of B (the
// wrapper checks).  ``chunk``: words per unit, rounded up to a multiple of 128 (0: enough units to fill the grid).
int alink_fpm_class_counts(const void* B, int64_t W, const int* prefix, int P, const int64_t* cls_ptr,
                           const int* ext_item, int64_t n_classes, void* counts, int64_t chunk, int grid,
                           hipStream_t stream) {
    return launch_walk<ItemsetStep>(B, W, prefix, P, cls_ptr, ext_item, n_classes, counts, chunk, grid, stream);
}

// counts int64 [candidates] must be zero on entry.  ``prefix`` and ``ext`` hold step codes 2 * item + s whose items
// lie in the rows of B (the wrapper checks); ``wbits``: bits per sequence field, 8, 16, 32 or 64.  ``chunk`` and
// ``grid`` as in alink_fpm_class_counts.
int alink_fpm_seq_counts(const void* B, int64_t W, const int* prefix, int P, const int64_t* cls_ptr, const int* ext,
                         int64_t n_classes, void* counts, int wbits, int64_t chunk, int grid, hipStream_t stream) {
    switch (wbits) {
        case 8: return launch_walk<SeqStep<8>>(B, W, prefix, P, cls_ptr, ext, n_classes, counts, chunk, grid, stream);
        case 16: return launch_walk<SeqStep<16>>(B, W, prefix, P, cls_ptr, ext, n_classes, counts, chunk, grid, stream);
        case 32: return launch_walk<SeqStep<32>>(B, W, prefix, P, cls_ptr, ext, n_classes, counts, chunk, grid, stream);
        case 64: return launch_walk<SeqStep<64>>(B, W, prefix, P, cls_ptr, ext, n_classes, counts, chunk, grid, stream);
    }
    return 1;
}

}  // extern "C"
