// java.util.Random (48-bit LCG) batch shuffles for the host runtime: the per-node feature shuffles of
// seriestree/DecisionTree.bagging (reference A/operator/common/tree/seriestree/DecisionTree.java), the same draws
// as common/jrandom.py JavaRandom.shuffle, for a whole tree level in one call instead of ~F Python calls per node.
#include <cmath>
#include <cstdint>

namespace {

constexpr uint64_t kMult = 0x5DEECE66DULL;
constexpr uint64_t kAdd = 0xBULL;
constexpr uint64_t kMask = (1ULL << 48) - 1;

inline int32_t next_bits(uint64_t& seed, int bits) {
    seed = (seed * kMult + kAdd) & kMask;
    return (int32_t)(uint32_t)(seed >> (48 - bits));
}

inline int32_t next_int(uint64_t& seed, int32_t bound) {
    if ((bound & -bound) == bound) return (int32_t)(((int64_t)bound * (int64_t)next_bits(seed, 31)) >> 31);
    while (true) {
        const int32_t bits = next_bits(seed, 31);
        const int32_t val = bits % bound;
        if ((int32_t)((uint32_t)bits - (uint32_t)val + (uint32_t)(bound - 1)) >= 0) return val;
    }
}

// nextDouble: ((next(26) << 27) + next(27)) * 2^-53
inline double next_double(uint64_t& seed) {
    const int64_t hi = next_bits(seed, 26), lo = next_bits(seed, 27);
    return (double)((hi << 27) + lo) * (1.0 / (double)(1LL << 53));
}

}  // namespace

extern "C" {

// Shuffle m rows of n int32 in place, row after row (Fisher-Yates from the end with nextInt(i + 1), swapping only
// when idx != i), continuing the generator state *seed (the scrambled 48-bit state).
void alink_java_shuffle_rows(uint64_t* seed, int32_t* rows, int64_t m, int32_t n) {
    uint64_t s = *seed;
    for (int64_t r = 0; r < m; ++r) {
        int32_t* a = rows + r * n;
        for (int32_t i = n - 1; i > 0; --i) {
            const int32_t idx = next_int(s, i + 1);
            if (idx == i) continue;
            const int32_t t = a[idx];
            a[idx] = a[i];
            a[i] = t;
        }
    }
    *seed = s;
}

// The next n values of nextGaussian (Marsaglia polar method, as common/jrandom.py JavaRandom.nextGaussian: the same
// libm log and sqrt, the same operation order), continuing the state *seed and the cached second value
// (*have_next, *next), and leaving both as n single calls would.
void alink_java_next_gaussians(uint64_t* seed, int32_t* have_next, double* next, double* out, int64_t n) {
    uint64_t s = *seed;
    int32_t have = *have_next;
    double cached = *next;
    for (int64_t i = 0; i < n; ++i) {
        if (have) {
            out[i] = cached;
            have = 0;
            continue;
        }
        double v1, v2, q;
        do {
            v1 = 2 * next_double(s) - 1;
            v2 = 2 * next_double(s) - 1;
            q = v1 * v1 + v2 * v2;
        } while (!(0 < q && q < 1));
        const double mul = std::sqrt(-2 * std::log(q) / q);
        cached = v2 * mul;
        have = 1;
        out[i] = v1 * mul;
    }
    *seed = s;
    *have_next = have;
    *next = cached;
}

}  // extern "C"
