// Cluster evaluation row pass (``ops/evalcluster.py``): every row against the k cluster means in one pass over the
// rows, all arithmetic fp64, no [n, k] buffer.  Output per row r: out[r] = [own, own^2, sil].
//
//   own  the distance of the row to the mean of its own cluster cid[r] (dist 0 EUCLIDEAN sqrt(sum (x - m)^2),
//        1 COSINE 1 - x.m / (|x| |m|), 1 where a norm is 0, 2 CITYBLOCK sum |x - m|);
//   sil  the closed-form silhouette of ClusterEvaluationUtil.calSilhouetteCoefficient from the dots x.m_j, the
//        cluster counts cnt_j and squared-norm sums n2_j: EUCLIDEAN dis_j = cnt_j |x|^2 - 2 cnt_j x.m_j + n2_j,
//        cur = dis_own / (cnt_own - 1), nb = min_{j != own} dis_j / max(cnt_j, 1) (taken as a product with the
//        reciprocal the wrapper rounded once per cluster: k divisions per row would cost as much as the dots at
//        small d); otherwise dis_j = 1 - x.m_j,
//        cur = dis_own cnt_own / (cnt_own - 1), nb = min_{j != own} dis_j; cur = 0 when cnt_own <= 1, nb = +inf
//        when there is no other cluster; sil = cur < nb ? 1 - cur / nb : nb / cur - 1, NaN -> 0.
//   A row whose cid is outside [0, k) gets [0, 0, 0] and no mean is read for it.
//
// * alink_evalcluster_rows_f64 — dense fp64 rows [n, d], 1 <= d <= 1024.  The k dots run on the
//   tile loop of dense64_mfma.h (the table is the cluster means; operand maps and image layout are described
//   there): 64 rows per workgroup, blocks of 16 NT clusters, dim chunks of 32, the image of
//   ``kmeans_dense64.centroid_image`` with the COSINE code (plain dots, accumulators start at 0).  d is zero-padded
//   in the registers; odd d and 8-byte-aligned rows take scalar loads (VEC = false).
//   The epilogue walks the lane's own 4 NT accumulators (clusters g + 4 q of each tile), then the four lane groups:
//   a min that skips j == cid and every j >= k, and the own-cluster dot picked out by index.  |x|^2 is summed per
//   lane in ascending dim order and combined by a fixed xor butterfly (16, 32) before the epilogue.
//   own comes from the row's registers against a gather of mean[cid] (32 contiguous bytes per lane and 16-dim
//   group, served by L2: the table is k d doubles), each lane adding in ascending dim order, the same butterfly
//   across the lane groups: the three outputs depend on the row alone, not on the grid or the row's wave.
//   Choices: LDS 4 NT KiB per workgroup (<= 32 KiB, so LDS never limits below 5 workgroups per CU); 256-thread
//   workgroups so that one staged block serves 64 rows; the grid is capped at 1024 workgroups that stride over the
//   row batches.
// * alink_evalcluster_rows_csr — CSR rows (int32 / int64 columns), one wave per row, on the row walk of csr_rows.h
//   (the table is the cluster means, transposed and padded, Mt [d, kp]; the lane / cluster map and the entry guard
//   are described there): per cluster block the walk gives the lane's dots and |x|^2, and this file keeps ev_dis,
//   the min, the own dot and ev_store.  Entries whose column is outside [0, d) add nothing, to the dots and to the
//   norms alike.
//   own never touches d elements: with the per-cluster |m|^2 and sum |m| (stat columns 3, 4)
//     EUCLIDEAN  sqrt(max(0, |m|^2 + sum_nz((x_j - m_j)^2 - m_j^2))),
//     CITYBLOCK  sum |m| + sum_nz(|x_j - m_j| - |m_j|),
//     COSINE     1 - x.m / (|x| |m|) from the own dot,
//   where m_j = Mt[j, cid] is one wave-uniform load per entry, taken through the walk's per-entry hook (own_terms)
//   during the first cluster block.  A row must store a column at most once.
//   Every lane walks the entries in stored order, so a row's values do not depend on the grid.
//   Choices: no LDS (the table rows are read once per entry, coalesced over the lanes); 4 rows per 256-thread
//   workgroup; up to 16384 workgroups striding over the rows.
// Non-finite rows are not guaranteed (a NaN dot is skipped by the min).  Plain C++ and vector stores only.
#include "csr_rows.h"
#include "dense64_mfma.h"

namespace {

using namespace d64;

constexpr int EV_STAT = 8;           // doubles per cluster record: cnt, n2, 1 / max(cnt, 1), |m|^2, sum |m|, padding

// dis_j of the closed form from the dot x.m_j
__device__ __forceinline__ double ev_dis(int dist, double dot, double xn, double cn, double n2) {
    return dist == 0 ? cn * xn - 2.0 * cn * dot + n2 : 1.0 - dot;
}

// [own, own^2, sil] of one row from its own distance, its own dis, the neighbour minimum and its cluster's count
__device__ __forceinline__ void ev_store(double* __restrict__ o, int dist, double own, double disown, double nb,
                                         double cn) {
    double cur = 0.0;
    if (cn > 1.0) cur = dist == 0 ? disown / (cn - 1.0) : disown * cn / (cn - 1.0);
    double sil = cur < nb ? 1.0 - cur / nb : nb / cur - 1.0;
    if (sil != sil) sil = 0.0;
    o[0] = own;
    o[1] = own * own;
    o[2] = sil;
}

// img: the mean image (dense64_mfma.h); mean [k, d]; stat [nblk * 16 NT, 8] = (cnt, n2, 1 / max(cnt, 1), ...), zero
// on the padded slots.  VEC: even d and 16-byte aligned X and mean (load_chunk).
template <int NT, bool VEC>
__global__ __launch_bounds__(64 * WAVES) void evalcluster_rows_f64_kernel(
        const double* __restrict__ X, int64_t n, int d, const int* __restrict__ cid, const double* __restrict__ img,
        const double* __restrict__ mean, const double* __restrict__ stat, int k, int nblk, int ndch, int dist,
        double* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) double cent[NT * 512];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int m = lane & 15, g = lane >> 4;
    const int64_t nbatch = (n + ROWS - 1) / ROWS;
    for (int64_t b = blockIdx.x; b < nbatch; b += gridDim.x) {
        const int64_t row = b * ROWS + wave * 16 + m;
        const bool row_ok = row < n;
        const double* __restrict__ xr = X + (row_ok ? row : 0) * (int64_t)d;
        const int own = row_ok ? cid[row] : -1;
        const bool own_ok = own >= 0 && own < k;
        const double* __restrict__ mr = mean + (own_ok ? own : 0) * (int64_t)d;
        double nb = __builtin_inf();
        double owndot = 0.0;            // x . mean[own], on the lane group that holds it
        double xn = 0.0;
        double a0 = 0.0, a1 = 0.0;      // own: sum (x - m)^2 | x.m | sum |x - m|;  a1: sum m^2 (COSINE)
        for (int cb = 0; cb < nblk; ++cb) {
            d4_t acc[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = d4_t{0.0, 0.0, 0.0, 0.0};
            xn = 0.0;
            for (int dc = 0; dc < ndch; ++dc) {
                // this lane's dims of the row (zero outside it)
                double xb[2][4];
                load_chunk<VEC>(xb, xr, row_ok, dc, g, d);
                if (cb == 0) {
                    // the same dims of the row's own mean; the sums run in ascending dim order within the lane
                    double mb[2][4];
                    load_chunk<VEC>(mb, mr, own_ok, dc, g, d);
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
#pragma unroll
                        for (int s = 0; s < 4; ++s) {
                            const double x = xb[u][s], mm = mb[u][s];
                            if (dist == 0) {
                                const double t = x - mm;
                                a0 = fma(t, t, a0);
                            } else if (dist == 1) {
                                a0 = fma(x, mm, a0);
                                a1 = fma(mm, mm, a1);
                            } else {
                                a0 += fabs(x - mm);
                            }
                        }
                    }
                }
                stage<NT>(cent, img, cb, ndch, dc);     // the mean block of this dim chunk
#pragma unroll
                for (int u = 0; u < 2; ++u) {
#pragma unroll
                    for (int s = 0; s < 4; ++s) xn = fma(xb[u][s], xb[u][s], xn);
                    mfma_group<NT>(acc, cent, xb[u], u, g, m);
                }
            }
            // |x|^2 of the whole row on every lane group
            xn = group_sum(xn);
            // the lane's own clusters: tile, then register
#pragma unroll
            for (int t = 0; t < NT; ++t) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int c = (cb * NT + t) * 16 + g + 4 * q;
                    const double dot = acc[t][q];
                    if (c == own) {
                        owndot = dot;
                    } else if (c < k) {
                        const double* __restrict__ sc = stat + EV_STAT * c;
                        double v = ev_dis(dist, dot, xn, sc[0], sc[1]);
                        if (dist == 0) v = v * sc[2];
                        if (v < nb) nb = v;
                    }
                }
            }
        }
        // across the four lane groups of a row (every other group holds owndot = 0)
#pragma unroll
        for (int o = 16; o < 64; o <<= 1) {
            const double ob = __shfl_xor(nb, o, 64);
            nb = ob < nb ? ob : nb;
        }
        owndot = group_sum(owndot);
        a0 = group_sum(a0);
        a1 = group_sum(a1);
        if (g == 0 && row_ok) {
            double* __restrict__ o = out + row * 3;
            if (!own_ok) {
                o[0] = 0.0;
                o[1] = 0.0;
                o[2] = 0.0;
            } else {
                const double cn = stat[EV_STAT * own], n2 = stat[EV_STAT * own + 1];
                double ownd;
                if (dist == 0) {
                    ownd = sqrt(a0);
                } else if (dist == 1) {
                    const double cross = sqrt(xn) * sqrt(a1);
                    ownd = cross > 0.0 ? 1.0 - a0 / cross : 1.0;
                } else {
                    ownd = a0;
                }
                ev_store(o, dist, ownd, ev_dis(dist, owndot, xn, cn, n2), nb, cn);
            }
        }
    }
}

// The hook of the CSR walk (csr_rows.h) that sums own's entry terms from m = Mt[c, own], one wave-uniform load per
// entry: (v - m)^2 - m^2 (dist 0) or |v - m| - |m| (dist 2).  A (0, 0.0) entry gives exactly 0 either way.
struct own_terms {
    bool on;            // the first cluster block's walk alone, EUCLIDEAN and CITYBLOCK
    int own, dist;
    double oacc;
    __device__ __forceinline__ double gather(const double* __restrict__ rowp) const { return on ? rowp[own] : 0.0; }
    __device__ __forceinline__ void fold(double v, double m) {
        if (on) {
            const double df = v - m;
            oacc += dist == 0 ? df * df - m * m : fabs(df) - fabs(m);
        }
    }
};

// Mt [d, kp]; stat [kp, 8] = (cnt, n2, 1 / max(cnt, 1), |m|^2, sum |m|, ...), zero on the padded clusters.
// NB, U: cluster blocks of 64 per pass and entries whose gathers are issued together (csr_rows.h).
template <int NB, int U, typename I>
__global__ __launch_bounds__(64 * csr::WAVES) void evalcluster_rows_csr_kernel(
        const int64_t* __restrict__ crow, const I* __restrict__ col, const double* __restrict__ val, int64_t n,
        int64_t d, const int* __restrict__ cid, const double* __restrict__ Mt, const double* __restrict__ stat, int k,
        int kp, int dist, double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = csr::item_stride();
    for (int64_t r = csr::first_item(); r < n; r += nw) {
        const int64_t s = crow[r], e = crow[r + 1];
        const int own = __builtin_amdgcn_readfirstlane(cid[r]);
        const bool own_ok = own >= 0 && own < k;
        double* __restrict__ o = out + r * 3;
        if (!own_ok) {
            if (lane == 0) {
                o[0] = 0.0;
                o[1] = 0.0;
                o[2] = 0.0;
            }
            continue;
        }
        double nb = __builtin_inf();
        double owndot = 0.0;
        double xn = 0.0;
        double oacc = 0.0;
        for (int cb = 0; cb < kp; cb += 64 * NB) {
            const auto w = csr::row_dots<NB, U, csr::NBMAX>(col, val, s, e, d, Mt, kp, cb, lane,
                                                            own_terms{dist != 1 && cb == 0, own, dist, oacc});
            xn = w.xn;
            oacc = w.hook.oacc;
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const int c = cb + 64 * b + lane;
                if ((NB < csr::NBMAX || cb + 64 * b < kp) && c < k) {
                    if (c == own) {
                        owndot = w.acc[b];
                    } else {
                        const double* __restrict__ sc = stat + EV_STAT * c;
                        double v = ev_dis(dist, w.acc[b], xn, sc[0], sc[1]);
                        if (dist == 0) v = v * sc[2];
                        if (v < nb) nb = v;
                    }
                }
            }
        }
        // over the wave: the minimum, and the own dot from the one lane that holds it (every other lane holds 0)
#pragma unroll
        for (int of = 32; of > 0; of >>= 1) {
            const double ob = __shfl_xor(nb, of, 64);
            nb = ob < nb ? ob : nb;
            owndot += __shfl_xor(owndot, of, 64);
        }
        if (lane == 0) {
            const double* __restrict__ so = stat + EV_STAT * own;
            const double cn = so[0], n2 = so[1], m2 = so[3], m1 = so[4];
            double ownd;
            if (dist == 0) {
                const double q = m2 + oacc;
                ownd = sqrt(q > 0.0 ? q : 0.0);
            } else if (dist == 1) {
                const double cross = sqrt(xn) * sqrt(m2);
                ownd = cross > 0.0 ? 1.0 - owndot / cross : 1.0;
            } else {
                ownd = m1 + oacc;
            }
            ev_store(o, dist, ownd, ev_dis(dist, owndot, xn, cn, n2), nb, cn);
        }
    }
}

}  // namespace

extern "C" {

// The row pass over n fp64 rows X [n, d] (1 <= d <= 1024, 8-byte aligned) with clusters cid int32 [n]: img is the
// mean image of ``ops/kmeans_dense64.centroid_image`` (COSINE code) for tiles-per-block nt (1, 2, 4 or 8), nblk
// blocks of 16 nt cluster slots; mean [k, d]; stat [nblk * 16 nt, 8] = the cluster records (cnt, n2,
// 1 / max(cnt, 1), |m|^2, sum |m|, 0, 0, 0; the dense kernel reads the first three), padded with zeros; dist 0
// EUCLIDEAN, 1 COSINE, 2 CITYBLOCK.  out [n, 3]: every element is written.
int alink_evalcluster_rows_f64(const double* X, int64_t n, int d, const int* cid, const double* img,
                               const double* mean, const double* stat, int k, int nt, int nblk, int dist, double* out,
                               int grid, void* stream) {
    if (n <= 0) return 0;
    if (d < 1 || d > 1024 || k < 1 || nblk < 1 || (int64_t)nblk * nt * 16 < k || n >= (1ll << 31)) return 1;
    if (!nt_ok(nt)) return 1;
    if (dist < 0 || dist > 2) return 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int ndch = (d + DCH - 1) / DCH;
    const bool vec = vec_ok(d, X) && vec_ok(d, mean);
    ALINK_D64_LAUNCH(evalcluster_rows_f64_kernel, nt, 1, 2, 4, 8, vec, row_blocks(n, grid, 1024), st, X, n, d, cid,
                     img, mean, stat, k, nblk, ndch, dist, out);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

// The row pass over n CSR rows (crow int64 [n+1]; col int32, or int64 with idx64; val fp64) under d columns with
// clusters cid int32 [n]: Mt [d, kp] the transposed means (kp a multiple of 64, k <= kp), stat [kp, 8] the same
// cluster records, padded with zeros; dist as above.  out [n, 3]: every element is written.
int alink_evalcluster_rows_csr(const int64_t* crow, const void* col, int idx64, const double* val, int64_t n,
                               int64_t d, const int* cid, const double* Mt, const double* stat, int k, int kp,
                               int dist, double* out, int grid, void* stream) {
    if (n <= 0) return 0;
    if (d < 1 || k < 1 || kp < 64 || kp % 64 != 0 || k > kp || n >= (1ll << 31)) return 1;
    if (dist < 0 || dist > 2) return 1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ALINK_CSR_LAUNCH(evalcluster_rows_csr_kernel, kp, idx64, csr::wave_blocks(n, grid, csr::WAVES, csr::WAVE_GRID), st,
                     crow, col, val, n, d, cid, Mt, stat, k, kp, dist, out);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}

}  // extern "C"
