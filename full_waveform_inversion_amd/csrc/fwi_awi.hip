// Adaptive (per-trace matching-filter) misfit of (nt, ntr) trace gathers (fwi_awi.h): per trace the normal equations of
// the Wiener filter from the lag correlations of fwi_ttime.hip, their dense solve, the filter's second moment and the
// adjoint source.  Its own object: the step / tile / point / smoothing / regularisation / data / matching / envelope /
// correlation / traveltime / transport / spectral objects keep their pinned kernel counts.
//
// awi_solve is the new hot one: ntr symmetric positive definite systems of K = 2 L + 1 <= 129 unknowns, two right-hand
// sides each, K^3 / 6 fp64 FMAs for the factor.  One workgroup per trace.  The lower triangle of G_j lies packed in LDS
// BY COLUMNS, G[i][j] (i >= j) at col(j) + i - j with col(j) = j K - j (j - 1) / 2: thread i owns row i, and wherever the
// threads of a wave read one column at their own rows the addresses are consecutive doubles (no bank conflict), while
// the second operand of every product is one address for the whole wave (a broadcast).  8385 doubles at L = 64, 67 KB,
// plus 2 KB of vectors: two workgroups share a CU's 160 KiB.
//   factor   left-looking, column j = 0 .. K - 1: thread i >= j forms G[i][j] - sum_{k < j} L[i][k] L[j][k] in a register,
//            by fma over ascending k; thread j takes the square root of its own (the pivot), the others divide by it.
//   solves   column-oriented, thread i keeps the i-th entry of the right-hand side in a register: forward, for k ascending
//            thread k divides by L[k][k] and publishes y_k, the threads i > k subtract L[i][k] y_k by fma; backward, for k
//            descending thread k divides and publishes x_k, the threads i < k subtract L[k][i] x_k.  Every entry thus
//            receives its terms one by one in a fixed order (ascending k forward, descending k backward).
//   moments  N_j and sum_k (k dt)^2 w_k^2 by one thread over ascending k.
// Nothing is added in an order that depends on timing, there are no atomics: equal inputs give equal bits.
//
// awi_source: lane = trace as in the shared gather tile (fwi_gather_tile.h), 64 traces by 32 output times per block, 8
// output times per thread in registers.  The z_k of the block's 64 traces are staged in LDS lag-major (lane-contiguous
// doubles); per lag a thread reads one z and one new dh value and slides a window of 8 dh values through its registers,
// 8 unrolled steps so that the window's slots rotate at compile time: 8 FMAs per LDS read and global load.
#include <hip/hip_runtime.h>

#include "fwi_awi.h"
#include "fwi_gather_tile.h"
#include "fwi_kernels.h"

namespace fwi {

namespace {

constexpr int AWI_BLOCK = 256;
constexpr int AWI_TRI = AWI_KMAX * (AWI_KMAX + 1) / 2;  // packed lower triangle
constexpr int AWI_KPAD = (AWI_KMAX + GT_TO - 1) / GT_TO * GT_TO;  // lags staged by awi_source: whole groups of 8
static_assert(AWI_KMAX <= AWI_BLOCK, "thread i owns row i");
static_assert(2 * (AWI_TRI + 2 * AWI_KPAD + 8) * sizeof(double) <= 163840, "two workgroups share a CU's LDS");
static_assert(2 * AWI_KPAD * GT_LANES * sizeof(double) <= 163840, "two blocks share a CU's LDS");

// thread i's entry v of the right-hand side -> its entry of G^-1 (rhs), G = L L^T the factor in sG; sv: K doubles of LDS
// through which the unknowns are published.  Called by every thread of the block (barriers inside).
__device__ __forceinline__ double awi_solve_one(double v, const double *sG, double *sv, int i, int K, int ci) {
    // L y = rhs
    for (int k = 0, ck = 0; k < K; ck += K - k, ++k) {  // ck = col(k)
        if (i == k) {
            v = v / sG[ck];
            sv[k] = v;
        }
        __syncthreads();
        if (i > k && i < K) v = fma(-sG[ck + i - k], sv[k], v);
    }
    // L^T x = y
    for (int k = K - 1; k >= 0; --k) {
        if (i == k) {
            v = v / sG[ci];
            sv[k] = v;
        }
        __syncthreads();
        if (i < k) v = fma(-sG[ci + k - i], sv[k], v);
    }
    return v;
}

__global__ __launch_bounds__(AWI_BLOCK) void awi_solve(double *work, int32_t *counts, const double *partC,
                                                       const double *partA, const double *tw, double dt, double lam, int L,
                                                       int Le, int slC, int Ae, int slA, int ntr) {
    __shared__ double sG[AWI_TRI];
    __shared__ double sa[AWI_KPAD];
    __shared__ double sv[AWI_KPAD];
    __shared__ double sd[4];  // the pivot of the column; N, W of the trace
    __shared__ int sbad, scnt;
    const int i = threadIdx.x, j = blockIdx.x, K = 2 * L + 1;
    const int nlagC = 2 * Le + 1, nlagA = 2 * Ae + 1;
    const int ci = i < K ? i * K - i * (i - 1) / 2 : 0;  // col(i)

    // a_j(m), m = 0 .. 2 L, and this thread's c_j(i - L): the slices in ascending order; lags beyond nt - 1 are 0
    if (i < K) {
        double a = 0.0;
        if (i <= Ae)
            for (int sl = 0; sl < slA; ++sl) a += partA[((int64_t)sl * nlagA + (i + Ae)) * ntr + j];
        sa[i] = a;
    }
    double rhs = 0.0;
    if (i < K && i - L >= -Le && i - L <= Le)
        for (int sl = 0; sl < slC; ++sl) rhs += partC[((int64_t)sl * nlagC + (i - L + Le)) * ntr + j];
    if (i == 0) sbad = 0;
    __syncthreads();
    const double a0 = sa[0];
    const bool alive = isfinite(a0) && a0 > 0.0;

    // G packed by columns
    for (int c = 0, cc = 0; c < K; cc += K - c, ++c)
        if (i >= c && i < K) sG[cc + i - c] = sa[i - c] + (i == c ? lam * a0 : 0.0);
    __syncthreads();

    // Cholesky, in place
    for (int c = 0, cc = 0; c < K; cc += K - c, ++c) {
        double s = 0.0;
        if (i >= c && i < K) {
            s = sG[cc + i - c];
            int q = i;  // col(k) + i - k
#pragma unroll 4
            for (int k = 0; k < c; ++k) {
                s = fma(-sG[q], sG[q - i + c], s);
                q += K - k - 1;
            }
        }
        if (i == c) {
            const bool good = isfinite(s) && s > 0.0;
            if (!good) sbad = 1;
            const double p = good ? sqrt(s) : 1.0;
            sG[cc] = p;
            sd[0] = p;
        }
        __syncthreads();
        if (i > c && i < K) sG[cc + i - c] = s / sd[0];
        __syncthreads();
    }

    const double wv = awi_solve_one(rhs, sG, sv, i, K, ci);  // w_j = G^-1 c_j

    if (i == 0) {
        double N = 0.0, S = 0.0;
        for (int k = 0; k < K; ++k) {
            const double t = (double)(k - L) * dt, w2 = sv[k] * sv[k];
            N += w2;
            S = fma(t * t, w2, S);
        }
        const bool cnt = alive && !sbad && isfinite(N) && N > 0.0 && isfinite(S);
        sd[1] = cnt ? N : 1.0;
        sd[2] = cnt ? S / N : 0.0;
        scnt = cnt ? 1 : 0;
    }
    __syncthreads();
    const bool cnt = scnt != 0;
    const double N = sd[1], W = sd[2], twj = tw ? tw[j] : 1.0;
    const double t = (double)(i - L) * dt;
    const double y = cnt ? twj * wv * (t * t - W) / N : 0.0;
    __syncthreads();  // sv is read: the second solve may write it

    const double zv = awi_solve_one(y, sG, sv, i, K, ci);  // z_j = G^-1 y_j

    if (i < K) {
        work[awi_w_at(ntr, L) + (size_t)j * K + i] = cnt ? wv : 0.0;
        work[awi_z_at(ntr, L) + (size_t)i * ntr + j] = cnt ? zv : 0.0;
    }
    if (i == 0) {
        work[awi_w2_at(ntr, L) + j] = W;
        work[awi_term_at(ntr, L) + j] = cnt ? 0.5 * twj * W : 0.0;
        counts[j] = cnt ? 1 : 0;
    }
}

template <typename T>
__global__ __launch_bounds__(GT_BLOCK) void awi_source(T *g, const T *d, const T *w, const double *z,
                                                       const int32_t *counts, int nt, int ntr, int L, int xtiles) {
    __shared__ double sZ[AWI_KPAD * GT_LANES];
    const GatherTile c = gather_tile(xtiles);
    const int K = 2 * L + 1, Kp = (K + GT_TO - 1) / GT_TO * GT_TO;
    // z_k of the tile's traces, lag-major; the lags from K on (the last group's padding) and traces >= ntr: zeros
    for (int i = threadIdx.x; i < Kp * GT_LANES; i += GT_BLOCK) {
        const int k = i >> 6, gx = c.x0 + (i & 63);
        sZ[i] = (k < K && gx < ntr) ? z[(size_t)k * ntr + gx] : 0.0;
    }
    __syncthreads();
    if (c.gx >= ntr) return;
    if (!counts[c.gx]) {
#pragma unroll
        for (int o = 0; o < GT_TO; ++o)
            if (c.tn0 + o < nt) g[(int64_t)(c.tn0 + o) * ntr + c.gx] = (T)0;
        return;
    }
    auto dh = [&](int row) -> double {  // (M d)[row, gx]; rows outside [0, nt) are not read: zeros
        if (row < 0 || row >= nt) return 0.0;
        const int64_t at = (int64_t)row * ntr + c.gx;
        return (w ? (double)w[at] : 1.0) * (double)d[at];
    };
    double acc[GT_TO], x[GT_TO];
    // at step t (lag k = t - L) output o pairs dh[tn0 + o - k]: slot (o - t) % 8 of the window
#pragma unroll
    for (int o = 0; o < GT_TO; ++o) acc[o] = 0.0, x[o] = dh(c.tn0 + o + L);
    const double *pz = sZ + c.lane;
#pragma unroll 1
    for (int tb = 0; tb < Kp; tb += GT_TO) {
        double nv[GT_TO];  // what enters the window after each of the 8 steps: dh[tn0 + L - t - 1]
#pragma unroll
        for (int u = 0; u < GT_TO; ++u) nv[u] = dh(c.tn0 + L - (tb + u) - 1);
#pragma unroll
        for (int u = 0; u < GT_TO; ++u) {
            const double zk = pz[(tb + u) * GT_LANES];
#pragma unroll
            for (int o = 0; o < GT_TO; ++o) acc[o] = fma(zk, x[(o - u + GT_TO) % GT_TO], acc[o]);
            x[(GT_TO - 1 - u) % GT_TO] = nv[u];
        }
    }
#pragma unroll
    for (int o = 0; o < GT_TO; ++o) {
        if (c.tn0 + o < nt) {
            const int64_t at = (int64_t)(c.tn0 + o) * ntr + c.gx;
            g[at] = (T)((w ? (double)w[at] : 1.0) * acc[o]);
        }
    }
}

bool awi_shape(int nt, int ntr, int L) {
    return nt >= 1 && ntr >= 1 && L >= 1 && L <= AWI_LMAX && gather_blocks(nt, ntr) <= 0x7fffffff;
}

}  // namespace

template <typename T>
hipError_t launch_awi_correlations(double *part, const T *s, const T *d, const T *w, int L, int nt, int ntr,
                                   hipStream_t st) {
    if (!part || !s || !d || !awi_shape(nt, ntr, L)) return hipErrorInvalidValue;
    hipError_t e = launch_tt_xcorr<T>(part, s, d, w, L, nt, ntr, st);
    if (e != hipSuccess) return e;
    return launch_tt_xcorr<T>(part + awi_part_a_at(nt, ntr, L), d, d, w, 2 * L, nt, ntr, st);
}

hipError_t launch_awi_solve(double *work, int32_t *counts, const double *part, const double *tw, double dt, double lam,
                            int L, int nt, int ntr, hipStream_t st) {
    if (!work || !counts || !part || !awi_shape(nt, ntr, L) || !(lam > 0.0)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(awi_solve, dim3((unsigned)ntr), dim3(AWI_BLOCK), 0, st, work, counts, part,
                       part + awi_part_a_at(nt, ntr, L), tw, dt, lam, L, tt_reach(nt, L), tt_slices(nt, ntr, L),
                       tt_reach(nt, 2 * L), tt_slices(nt, ntr, 2 * L), ntr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_sum_partials(work + awi_term_at(ntr, L), ntr, st);
}

template <typename T>
hipError_t launch_awi_source(T *g, const T *d, const T *w, const double *work, const int32_t *counts, int L, int nt,
                             int ntr, hipStream_t st) {
    if (!g || !d || !work || !counts || !awi_shape(nt, ntr, L) || g == d || g == w) return hipErrorInvalidValue;
    hipLaunchKernelGGL(awi_source<T>, dim3((unsigned)gather_blocks(nt, ntr)), dim3(GT_BLOCK), 0, st, g, d, w,
                       work + awi_z_at(ntr, L), counts, nt, ntr, L, gather_xtiles(ntr));
    return hipGetLastError();
}

template hipError_t launch_awi_correlations<float>(double *, const float *, const float *, const float *, int, int, int,
                                                   hipStream_t);
template hipError_t launch_awi_correlations<double>(double *, const double *, const double *, const double *, int, int,
                                                    int, hipStream_t);
template hipError_t launch_awi_source<float>(float *, const float *, const float *, const double *, const int32_t *, int,
                                             int, int, hipStream_t);
template hipError_t launch_awi_source<double>(double *, const double *, const double *, const double *, const int32_t *,
                                              int, int, int, hipStream_t);

}  // namespace fwi
