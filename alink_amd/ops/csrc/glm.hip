// Generalized linear models on gfx950 / MI355X: the IRLS statistics pass and the per-row pass of
// models/regression/glm.py, for contiguous fp64 rows X [n, k] with 1 <= k <= GLM_KMAX = 126 (ops/glm.py).
//
// alink_glm_irls_f64: one pass over X that gives [sum ww^2 | G], G = sum_i ww_i a_i a_i^T over the augmented rows
// a_i = [x_i | 1 | z_i] (KA = k + 2 <= 128 entries, NT = ceil(KA / 16) tiles), z and ww the working label and weight
// of the mode (PLAIN, INIT, STEP).  A workgroup of 4 waves owns one row chunk and walks it 64 rows at a time:
//   load    four lanes per row (tid >> 2 the row, tid & 3 = sub) read the row from HBM once, lane sub the column
//           pairs 8 j + 2 sub (one 16-byte load where k is even and X 16-byte aligned, two 8-byte loads otherwise),
//           dot them with beta (LDS) by fma in ascending j, and store them to the row's LDS slot; the columns behind
//           KA are zero.  Two xor steps add the four lanes, so eta has the same bits on every path.
//   family  lane sub = 0 evaluates family and link (a wave-uniform switch on run-time ids) and writes z into the
//           row's column k + 1 and ww beside the rows.
//   Gram    after one barrier, the weighted upper tile triangle of gram64_mfma.h (the operand maps, which wave owns
//           which tile and the order of every addition are described there): at most 9 accumulator tiles per wave.
//   merge   part [nchunk, 1 + KA KA] holds each chunk's sum ww^2 and the entries of its upper tiles, merged in chunk
//           order with the mirror map of ordered_sum.h: the same bits for every grid and run.
//
// alink_glm_rows_f64: the same row load and dot without the LDS staging, then by mask: pred (mu), eta, the four
// residuals, z and ww, and per 64-row batch one partial of [deviance, deviance at unlink(cnull + off), pearson^2, w],
// merged in segments of 4096 batches and then by one workgroup, a rule that depends on the batch count alone.
//
// All arithmetic is fp64 and follows the torch formulas of glm.py operation for operation (no contraction: the only
// fused operations are the explicit fma of the dot and the matrix instruction).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gram64_mfma.h"
#include "ordered_sum.h"

#pragma clang fp contract(off)

namespace {

using d64::d2_t;
using d64::d4_t;
using d64::row_dot;
using d64::stage_beta;

constexpr double EPSILON = 1e-16, DELTA = 0.1, JAVA_MAX_VALUE = 1.7976931348623157e308, JAVA_MIN_VALUE = 4.9e-324;
constexpr int GLM_KMAX = 126;
constexpr int GLM_RED = 1024;       // threads of the sums reduction
constexpr int GLM_SEG = 4096;       // batch partials per workgroup of its first level (ops/glm.py sizes part by it)
enum { GAUSSIAN = 0, BINOMIAL, POISSON, GAMMA, TWEEDIE };
enum { L_IDENTITY = 0, L_LOG, L_LOGIT, L_INVERSE, L_SQRT, L_CLOGLOG, L_POWER };
enum { PLAIN = 0, INIT, STEP };
enum { M_PRED = 1, M_ETA = 2, M_RES = 4, M_ZW = 8, M_SUMS = 16 };

struct Fl {
    int fam, link;
    double vp, lp;
};

// torch.pow(x, p) with a scalar exponent: the special cases torch takes before the general pow, so that tweedie's
// default variancePower 1.5 (exponents -0.5 and 0.5) and the inverse-square links round as the torch path does
__device__ __forceinline__ double t_pow(double x, double p) {
    if (p == 0.5) return sqrt(x);
    if (p == -0.5) return 1.0 / sqrt(x);
    if (p == 2.0) return x * x;
    if (p == 3.0) return x * x * x;
    if (p == -1.0) return 1.0 / x;
    if (p == -2.0) return 1.0 / (x * x);
    if (p == 1.0) return x;
    if (p == 0.0) return 1.0;
    return pow(x, p);
}

__device__ __forceinline__ double f_link(const Fl& f, double mu) {
    switch (f.link) {
        case L_LOG: return log(mu);
        case L_LOGIT: return log(mu / (1.0 - mu));
        case L_INVERSE: return 1.0 / mu;
        case L_SQRT: return sqrt(mu);
        case L_CLOGLOG: return log(-log(1.0 - mu));
        case L_POWER: return f.lp == 0.0 ? log(mu) : t_pow(mu, f.lp);
        default: return mu;
    }
}

__device__ __forceinline__ double f_unlink(const Fl& f, double eta) {
    switch (f.link) {
        case L_LOG: return exp(eta);
        case L_LOGIT: return 1.0 / (1.0 + exp(-eta));
        case L_INVERSE: return 1.0 / eta;
        case L_SQRT: return eta * eta;
        case L_CLOGLOG: return 1.0 - exp(-exp(eta));
        case L_POWER: return f.lp == 0.0 ? exp(eta) : t_pow(eta, 1.0 / f.lp);
        default: return eta;
    }
}

__device__ __forceinline__ double f_deriv(const Fl& f, double mu) {
    switch (f.link) {
        case L_LOG: return 1.0 / mu;
        case L_LOGIT: return 1.0 / (mu * (1.0 - mu));
        case L_INVERSE: return -(1.0 / (mu * mu));          // torch.pow(mu, -2.0)
        case L_SQRT: return 1.0 / (2.0 * sqrt(mu));
        case L_CLOGLOG: return 1.0 / ((mu - 1.0) * log(1.0 - mu));
        case L_POWER: return f.lp == 0.0 ? 1.0 / mu : f.lp * t_pow(mu, f.lp - 1.0);
        default: return 1.0;
    }
}

// the comparisons are written so that a NaN passes through, as torch.where / clamp leave it
__device__ __forceinline__ double f_project(const Fl& f, double mu) {
    if (f.fam == GAUSSIAN) {
        if (mu == INFINITY) mu = JAVA_MAX_VALUE;
        return mu == -INFINITY ? JAVA_MIN_VALUE : mu;
    }
    if (f.fam == BINOMIAL) return mu < EPSILON ? EPSILON : (mu > 1.0 - EPSILON ? 1.0 - EPSILON : mu);
    if (mu < EPSILON) mu = EPSILON;
    return isinf(mu) ? JAVA_MAX_VALUE : mu;
}

__device__ __forceinline__ double f_variance(const Fl& f, double mu) {
    switch (f.fam) {
        case BINOMIAL: return mu * (1.0 - mu);
        case POISSON: return mu;
        case GAMMA: return mu * mu;
        case TWEEDIE: return t_pow(mu, f.vp);
        default: return 1.0;
    }
}

__device__ __forceinline__ double f_initialize(const Fl& f, double y, double w) {
    switch (f.fam) {
        case BINOMIAL: return (w * y + 0.5) / (w + 1.0);
        case POISSON: return y < DELTA ? DELTA : y;
        case TWEEDIE: return y == 0.0 ? DELTA : y;
        default: return y;
    }
}

__device__ __forceinline__ double ylogy(double a, double b) { return a == 0.0 ? 0.0 : a * log(a / b); }

__device__ __forceinline__ double f_deviance(const Fl& f, double y, double mu, double w) {
    switch (f.fam) {
        case BINOMIAL: return 2.0 * w * (ylogy(y, mu) + ylogy(1.0 - y, 1.0 - mu));
        case POISSON: return 2.0 * w * (ylogy(y, mu) - (y - mu));
        case GAMMA: return -2.0 * w * (log(y / mu) - (y - mu) / mu);
        case TWEEDIE: {
            const double y1 = y == 0.0 ? 1.0 : y;
            const double p1 = 1.0 - f.vp, p2 = 2.0 - f.vp;
            const double theta = f.vp == 1.0 ? log(y1 / mu) : (t_pow(y1, p1) - t_pow(mu, p1)) / p1;
            const double kappa = f.vp == 2.0 ? log(y1 / mu) : (t_pow(y, p2) - t_pow(mu, p2)) / p2;
            const double d = 2.0 * w * (y * theta - kappa);
            return d < EPSILON ? EPSILON : d;
        }
        default: return w * (y - mu) * (y - mu);
    }
}

// the working label and weight of one row
__device__ __forceinline__ void f_working(const Fl& f, int mode, double eta, double y, double w, double o, double& z,
                                          double& ww) {
    if (mode == STEP) {
        const double mu = f_project(f, f_unlink(f, eta));
        const double g = f_deriv(f, mu);
        z = eta - o + (y - mu) * g;
        ww = w / (g * g * f_variance(f, mu));
    } else if (mode == INIT) {
        z = f_link(f, f_project(f, f_initialize(f, y, w))) - o;
        ww = w;
    } else {
        z = y - o;
        ww = w;
    }
}

// pc = the chunk's [sum ww^2 | G [ka, ka]]: acc[s][q] = G[16 ta + g + 4 q][16 tb + m] of slot s's tile
template <int NT>
struct GramStore {
    using G = d64::GramTiles<NT, true, false>;
    template <int WAVE, int s = 0>
    static __device__ __forceinline__ void store(const d4_t (&acc)[G::MAXT], double* __restrict__ pc, int ka, int g,
                                                 int m) {
        if constexpr (s < G::MAXT) {
            constexpr int t = G::tile(WAVE, s);
            if constexpr (t < G::TU) {
                constexpr int ta = d64::tile_a(NT, t), tb = d64::tile_b(NT, t);
                const int cb = 16 * tb + m;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int ra = 16 * ta + g + 4 * q;
                    if (ra < ka && cb < ka) pc[1 + (int64_t)ra * ka + cb] = acc[s][q];
                }
            }
            store<WAVE, s + 1>(acc, pc, ka, g, m);
        }
    }
};

// The second bound is waves per SIMD; with workgroups of 4 waves, one per SIMD, it is also workgroups per CU.  Two at
// NT = 5: the LDS allows them at every NT <= 6 and the registers do up to NT = 4 unasked; at NT = 5 the compiler has to
// be told, or it takes 244 + 32 registers and one (profiles/gram_shared_triangle.txt).  A compiler that chooses
// otherwise may need another NT in the condition: the profile's table of occupancies is the check.
template <int NT, bool VEC>
__global__ __launch_bounds__(256, NT == 5 ? 2 : 1) void glm_irls_kernel(
        const double* __restrict__ X, const double* __restrict__ y, const double* __restrict__ w,
        const double* __restrict__ off, int64_t n, int k, const double* __restrict__ beta, double b0, Fl f, int mode,
        int64_t chunk_rows, int64_t nchunk, double* __restrict__ part) {
    using G = d64::GramTiles<NT, true, false>;
    constexpr int S = G::S;
    __shared__ __attribute__((aligned(16))) double rows[64 * S];
    __shared__ __attribute__((aligned(16))) double bet[128];
    __shared__ double wws[64];
    __shared__ __attribute__((aligned(32))) double red[G::RED];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = tid >> 2, sub = tid & 3;
    const int m = lane & 15, g = lane >> 4;
    const int ka = k + 2;
    const int64_t P = 1 + (int64_t)ka * ka;
    stage_beta(bet, mode == STEP ? beta : nullptr, k);
    for (int64_t c = blockIdx.x; c < nchunk; c += gridDim.x) {
        const int64_t r0 = c * chunk_rows;
        const int64_t r1 = r0 + chunk_rows < n ? r0 + chunk_rows : n;
        d4_t acc[G::MAXT];
#pragma unroll
        for (int s = 0; s < G::MAXT; ++s) acc[s] = d4_t{0.0, 0.0, 0.0, 0.0};
        double sww = 0.0;
        for (int64_t bb = r0; bb < r1; bb += 64) {
            const int64_t i = bb + r;
            const bool ok = i < r1;
            d2_t v[2 * NT];
            const double dot = row_dot<NT, VEC>(X + (ok ? i : r0) * (int64_t)k, ok, k, sub, bet, v);
            double* __restrict__ slot = rows + r * S;
#pragma unroll
            for (int j = 0; j < 2 * NT; ++j) {
                const int cc = 8 * j + 2 * sub;
                d2_t t = v[j];
                if (ok && cc == k) t[0] = 1.0;
                if (ok && cc + 1 == k) t[1] = 1.0;
                *reinterpret_cast<d2_t*>(slot + cc) = t;
            }
            if (sub == 0) {
                double z = 0.0, ww = 0.0;
                if (ok) {
                    const double o = off[i];
                    f_working(f, mode, dot + b0 + o, y[i], w[i], o, z, ww);
                }
                slot[k + 1] = z;        // after this wave's zero store of that pair, in program order
                wws[r] = ww;
            }
            __syncthreads();
            if (wave == 0) {
                const double a = wws[lane];
                sww += osum::wave_sum_desc(a * a);
            }
            G::batch(acc, rows, wws, wave, g, m);
            __syncthreads();        // the batch's reads are done before the next one is staged
        }
        double* __restrict__ pc = part + c * P;
        if (tid == 0) pc[0] = sww;
        G::template finish<GramStore<NT>>(acc, red, wave, lane, pc, ka, g, m);
    }
}

template <int NT, bool VEC>
__global__ __launch_bounds__(256) void glm_rows_kernel(
        const double* __restrict__ X, const double* __restrict__ y, const double* __restrict__ w,
        const double* __restrict__ off, int64_t n, int k, const double* __restrict__ beta, double b0, Fl f, int mode,
        int mask, double cnull, double* __restrict__ out, double* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) double bet[128];
    __shared__ double ws[4][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = tid >> 2, sub = tid & 3;
    stage_beta(bet, beta, k);
    const int64_t nb = (n + 63) / 64;
    for (int64_t b = blockIdx.x; b < nb; b += gridDim.x) {
        const int64_t i = b * 64 + r;
        const bool ok = i < n;
        d2_t v[2 * NT];
        const double dot = row_dot<NT, VEC>(X + (ok ? i : 0) * (int64_t)k, ok, k, sub, bet, v);
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        if (sub == 0 && ok) {
            const double o = off != nullptr ? off[i] : 0.0;
            const double eta = dot + b0 + o;
            const double mu = f_project(f, f_unlink(f, eta));
            int64_t at = i;         // the next column's slot of this row; out is touched under a column mask only
            if (mask & M_PRED) {
                out[at] = mu;
                at += n;
            }
            if (mask & M_ETA) {
                out[at] = eta;
                at += n;
            }
            if (mask & (M_RES | M_ZW | M_SUMS)) {
                const double yi = y[i], wi = w[i];
                const double dev = f_deviance(f, yi, mu, wi);
                const double pr = (yi - mu) * sqrt(wi) / sqrt(f_variance(f, mu));
                if (mask & M_RES) {
                    const double dr = sqrt(dev < 0.0 ? 0.0 : dev);
                    out[at] = yi <= mu ? -dr : dr;
                    out[at + n] = pr;
                    out[at + 2 * n] = (yi - mu) * f_deriv(f, mu);
                    out[at + 3 * n] = yi - mu;
                    at += 4 * n;
                }
                if (mask & M_ZW) {
                    double z, ww;
                    f_working(f, mode, eta, yi, wi, o, z, ww);
                    out[at] = z;
                    out[at + n] = ww;
                }
                if (mask & M_SUMS) {
                    s[0] = dev;
                    s[1] = f_deviance(f, yi, f_unlink(f, cnull + o), wi);
                    s[2] = pr * pr;
                    s[3] = wi;
                }
            }
        }
        if (mask & M_SUMS) {        // one partial per batch: the wave's rows by xor steps, the waves in order
#pragma unroll
            for (int q = 0; q < 4; ++q) s[q] = osum::wave_sum_desc(s[q]);
            if (lane == 0) {
#pragma unroll
                for (int q = 0; q < 4; ++q) ws[wave][q] = s[q];
            }
            __syncthreads();
            if (tid < 4) part[b * 4 + tid] = ((ws[0][tid] + ws[1][tid]) + ws[2][tid]) + ws[3][tid];
            __syncthreads();
        }
    }
}

// out [4 gridDim] = per workgroup the sums of its segment of seg rows of part [nb, 4] (a rule of the segment's length
// alone): the batches' partials in segments of GLM_SEG, then the segments' sums by one workgroup
__global__ __launch_bounds__(GLM_RED) void glm_sums_kernel(const double* __restrict__ part, int64_t nb, int64_t seg,
                                                           double* __restrict__ out) {
    __shared__ double sh[GLM_RED];
    const int tid = threadIdx.x, q = tid & 3;
    const int64_t i0 = (int64_t)blockIdx.x * seg;
    const int64_t i1 = i0 + seg < nb ? i0 + seg : nb;
    double a = 0.0;
    for (int64_t i = i0 + (tid >> 2); i < i1; i += GLM_RED / 4) a += part[i * 4 + q];
    sh[tid] = a;
    __syncthreads();
    for (int o = GLM_RED / 2; o >= 4; o >>= 1) {
        if (tid < o) sh[tid] += sh[tid + o];
        __syncthreads();
    }
    if (tid < 4) out[(int64_t)blockIdx.x * 4 + tid] = sh[tid];
}

bool ids_ok(int fam, int link, int mode) {
    return fam >= GAUSSIAN && fam <= TWEEDIE && link >= L_IDENTITY && link <= L_POWER && mode >= PLAIN && mode <= STEP;
}

}  // namespace

extern "C" {

// One IRLS statistics pass over X [n, k] (1 <= k <= 126), y, w, off [n]: out [1 + (k + 2)^2] = [sum ww^2 | G] through
// nchunk = ceil(n / chunk_rows) row chunks (chunk_rows a multiple of 64) whose partials part [nchunk, 1 + (k + 2)^2]
// are merged in chunk order.  fam / link / mode: the ids of ops/glm.py; beta [k] and b0 are read in mode STEP only.
int alink_glm_irls_f64(const double* X, const double* y, const double* w, const double* off, int64_t n, int k,
                       const double* beta, double b0, int fam, int link, double vp, double lp, int mode,
                       int64_t chunk_rows, int64_t nchunk, double* part, double* out, int grid, void* stream) {
    if (n <= 0) return 0;
    if (k < 1 || k > GLM_KMAX || n >= (1ll << 31) || !ids_ok(fam, link, mode)) return 1;
    if (chunk_rows < 64 || chunk_rows % 64 != 0 || nchunk != (n + chunk_rows - 1) / chunk_rows) return 1;
    if (X == nullptr || y == nullptr || w == nullptr || off == nullptr || part == nullptr || out == nullptr) return 1;
    if (mode == STEP && beta == nullptr) return 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int ka = k + 2, nt = (ka + 15) / 16;
    const Fl f{fam, link, vp, lp};
    const unsigned blocks = (unsigned)(grid > 0 && grid < nchunk ? grid : nchunk);
    ALINK_D64_LAUNCH_NT8(glm_irls_kernel, nt, d64::vec_ok(k, X), blocks, st, X, y, w, off, n, k, beta, b0, f, mode,
                         chunk_rows, nchunk, part);
    osum::chunk_merge(osum::GramMirror{1, ka}, 1 + (int64_t)ka * ka, nchunk, part, out, st);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

// The per-row pass: eta = x . beta + b0 + off (off may be null: 0), mu = project(unlink(eta)), and by mask the
// columns of out [ncol, n] in this order: 1 pred (mu), 2 eta, 4 the deviance / pearson / working / response residuals,
// 8 z and ww of `mode`; 16: sums [4] = [deviance, deviance at unlink(cnull + off), pearson^2, w] through
// part [nb + ceil(nb / 4096), 4], nb = ceil(n / 64): one partial per batch, then one per 4096 batches.  y and w are read by the masks 4, 8 and 16 only.
int alink_glm_rows_f64(const double* X, const double* y, const double* w, const double* off, int64_t n, int k,
                       const double* beta, double b0, int fam, int link, double vp, double lp, int mode, int mask,
                       double cnull, double* out, double* part, double* sums, int grid, void* stream) {
    if (n <= 0) return 0;
    if (k < 1 || k > GLM_KMAX || n >= (1ll << 31) || !ids_ok(fam, link, mode) || X == nullptr || beta == nullptr)
        return 1;
    if (mask <= 0 || mask >= 32) return 1;
    if ((mask & (M_RES | M_ZW | M_SUMS)) && (y == nullptr || w == nullptr)) return 1;
    if ((mask & (M_PRED | M_ETA | M_RES | M_ZW)) && out == nullptr) return 1;
    if ((mask & M_SUMS) && (part == nullptr || sums == nullptr)) return 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int nt = (k + 2 + 15) / 16;
    const Fl f{fam, link, vp, lp};
    ALINK_D64_LAUNCH_NT8(glm_rows_kernel, nt, d64::vec_ok(k, X), d64::row_blocks(n, grid, 8192), st, X, y, w, off, n,
                         k, beta, b0, f, mode, mask, cnull, out, part);
    if (mask & M_SUMS) {
        const int64_t nb = (n + 63) / 64, nseg = (nb + GLM_SEG - 1) / GLM_SEG;
        double* segs = part + nb * 4;
        if (nseg > 1)
            hipLaunchKernelGGL(glm_sums_kernel, dim3((unsigned)nseg), dim3(GLM_RED), 0, st, part, nb, (int64_t)GLM_SEG,
                               segs);
        hipLaunchKernelGGL(glm_sums_kernel, dim3(1), dim3(GLM_RED), 0, st, nseg > 1 ? segs : part,
                           nseg > 1 ? nseg : nb, nseg > 1 ? nseg : nb, sums);
    }
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // extern "C"
