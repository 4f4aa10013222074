// Cross-correlation traveltime misfit of (nt, ntr) trace gathers (fwi_ttime.h): the correlation of every trace pair
// over a window of lags, the pick with its parabolic refinement and the terms of J, and the adjoint source.  Its own
// object: the step / tile / point / smoothing / regularisation / data / matching / envelope / correlation objects keep
// their pinned kernel counts.
//
// tt_xcorr is the hot one, nt ntr (2 Ke + 1) fp64 FMAs.  Lane = trace as in the shared gather tile
// (fwi_gather_tile.h), but what a block of 256 threads owns besides its 64 traces is 32 consecutive LAGS, 8 per wave and
// lane in registers, and what it marches over is a slice of the time axis, in chunks of TT_CH rows staged through LDS as
// fp64 with the weights applied: the chunk's TT_CH rows of dh and the TT_CH + 31 rows of sh its lags reach.  Per time
// step a thread reads one dh value and one new sh value and slides a window of 8 sh values through its registers: 8
// FMAs for 2 LDS reads of lane-contiguous doubles (no bank conflict).  Eight steps are unrolled so that the window's
// slots rotate at compile time (a dynamically indexed local would go to LDS: DESIGN.md finding 0b).  For every (slice,
// lag, trace) the terms are added by fma over ascending time; tt_pick adds the slices in ascending order.  No atomics:
// equal inputs give equal bits.  All arithmetic between the loads and the one rounding of g to T is fp64.
#include <hip/hip_runtime.h>

#include "fwi_gather_tile.h"
#include "fwi_kernels.h"
#include "fwi_ttime.h"

namespace fwi {

namespace {

constexpr int TT_WL = TT_LAGS / (GT_BLOCK / GT_LANES);  // lags per wave and lane
constexpr int TT_SROWS = TT_CH + TT_LAGS;               // rows of sh in LDS: TT_CH + TT_LAGS - 1 used, one of padding
constexpr int TT_PBLOCK = 256;
static_assert(TT_WL == 8 && TT_CH % TT_WL == 0, "the window of 8 lags rotates once per 8 unrolled steps");
static_assert((TT_CH + TT_SROWS) * GT_LANES * sizeof(double) <= 65536, "two blocks share a CU's LDS");

template <typename T>
__global__ __launch_bounds__(GT_BLOCK) void tt_xcorr(double *part, const T *s, const T *d, const T *w, int nt, int ntr,
                                                     int Ke, int slen) {
    __shared__ double sD[TT_CH * GT_LANES];
    __shared__ double sS[TT_SROWS * GT_LANES];
    const int tid = threadIdx.x, lane = tid & 63, grp = tid >> 6;
    const int x0 = (int)blockIdx.x * GT_LANES;
    const int kb = (int)blockIdx.y * TT_LAGS - Ke;  // the block's first lag
    const int n_lo = (int)blockIdx.z * slen, n_hi = n_lo + slen < nt ? n_lo + slen : nt;
    double acc[TT_WL];
#pragma unroll
    for (int i = 0; i < TT_WL; ++i) acc[i] = 0.0;

    for (int m0 = n_lo; m0 < n_hi; m0 += TT_CH) {
        __syncthreads();  // the chunk before is used up
        // dh rows m0 .. m0 + TT_CH - 1 of the slice; rows >= n_hi and traces >= ntr are not read: zeros
        for (int i = tid; i < TT_CH * GT_LANES; i += GT_BLOCK) {
            const int row = m0 + (i >> 6), g = x0 + (i & 63);
            double v = 0.0;
            if (row < n_hi && g < ntr) {
                const int64_t at = (int64_t)row * ntr + g;
                v = (w ? (double)w[at] : 1.0) * (double)d[at];
            }
            sD[i] = v;
        }
        // sh rows m0 + kb .. m0 + kb + TT_CH + TT_LAGS - 2; rows outside [0, nt) are not read: zeros (the last slot is
        // padding that the window's final slide loads and nothing uses)
        for (int i = tid; i < TT_SROWS * GT_LANES; i += GT_BLOCK) {
            const int r = i >> 6, row = m0 + kb + r, g = x0 + (i & 63);
            double v = 0.0;
            if (r < TT_SROWS - 1 && row >= 0 && row < nt && g < ntr) {
                const int64_t at = (int64_t)row * ntr + g;
                v = (w ? (double)w[at] : 1.0) * (double)s[at];
            }
            sS[i] = v;
        }
        __syncthreads();
        const double *pd = sD + lane, *ps = sS + grp * TT_WL * GT_LANES + lane;
        double x[TT_WL];  // sh[n + k], k the wave's 8 lags: slot (t + i) % 8 holds lag i at step t of a group of 8
#pragma unroll
        for (int i = 0; i < TT_WL; ++i) x[i] = ps[i * GT_LANES];
#pragma unroll 1
        for (int tb = 0; tb < TT_CH; tb += TT_WL) {
            if (m0 + tb >= n_hi) break;  // (the same for the whole block)
#pragma unroll
            for (int t = 0; t < TT_WL; ++t) {
                const double dv = pd[(tb + t) * GT_LANES];
#pragma unroll
                for (int i = 0; i < TT_WL; ++i) acc[i] = fma(x[(t + i) % TT_WL], dv, acc[i]);
                x[t] = ps[(tb + t + TT_WL) * GT_LANES];
            }
        }
    }
    const int nlag = 2 * Ke + 1, gx = x0 + lane;
    if (gx < ntr) {
#pragma unroll
        for (int i = 0; i < TT_WL; ++i) {
            const int q = (int)blockIdx.y * TT_LAGS + grp * TT_WL + i;
            if (q < nlag) part[((int64_t)blockIdx.z * nlag + q) * ntr + gx] = acc[i];
        }
    }
}

__global__ __launch_bounds__(TT_PBLOCK) void tt_pick(double *coef, int32_t *lag, double *jterm, const double *part,
                                                     const double *tw, double dt, int Ke, int slices, int ntr) {
    const int j = blockIdx.x * TT_PBLOCK + threadIdx.x;
    if (j >= ntr) return;
    const int nlag = 2 * Ke + 1;
    double best = 0.0, cm = 0.0, cp = 0.0, prev = 0.0;
    int bq = 0;
    for (int q = 0; q < nlag; ++q) {
        double c = 0.0;
        for (int sl = 0; sl < slices; ++sl) c += part[((int64_t)sl * nlag + q) * ntr + j];
        if (q == 0 || c > best) {
            best = c, bq = q, cm = prev, cp = 0.0;
        } else if (q == bq + 1) {
            cp = c;
        }
        prev = c;
    }
    const double wj = tw ? tw[j] : 1.0;
    const double N = cm - cp, Q = cm - 2.0 * best + cp;
    double tau = 0.0, am = 0.0, a0 = 0.0, ap = 0.0, term = 0.0;
    if (bq > 0 && bq < nlag - 1 && best > 0.0 && Q < 0.0) {  // the trace counts
        tau = ((double)(bq - Ke) + N / (2.0 * Q)) * dt;
        const double a = wj * tau * dt, q2 = Q * Q;
        am = a * ((Q - N) / (2.0 * q2));
        a0 = a * (N / q2);
        ap = a * ((-Q - N) / (2.0 * q2));
        term = 0.5 * wj * (tau * tau);
    }
    lag[j] = bq - Ke;
    coef[j] = tau;
    coef[(int64_t)ntr + j] = am;
    coef[2 * (int64_t)ntr + j] = a0;
    coef[3 * (int64_t)ntr + j] = ap;
    jterm[j] = term;
}

template <typename T>
__global__ __launch_bounds__(GT_BLOCK) void tt_source(T *g, const T *d, const T *w, const double *coef,
                                                      const int32_t *lag, int nt, int ntr, int xtiles) {
    const GatherTile c = gather_tile(xtiles);
    if (c.gx >= ntr) return;
    const double am = coef[(int64_t)ntr + c.gx], a0 = coef[2 * (int64_t)ntr + c.gx], ap = coef[3 * (int64_t)ntr + c.gx];
    const int ks = lag[c.gx];
    // dh at the rows tn0 - k* - 1 .. tn0 - k* + 8 that the thread's 8 outputs pair: each read once
    double dh[GT_TO + 2];
#pragma unroll
    for (int i = 0; i < GT_TO + 2; ++i) {
        const int row = c.tn0 - ks - 1 + i;
        dh[i] = 0.0;
        if (row >= 0 && row < nt) {
            const int64_t at = (int64_t)row * ntr + c.gx;
            dh[i] = (w ? (double)w[at] : 1.0) * (double)d[at];
        }
    }
#pragma unroll
    for (int j = 0; j < GT_TO; ++j) {
        if (c.tn0 + j < nt) {
            const int64_t at = (int64_t)(c.tn0 + j) * ntr + c.gx;
            const double m = w ? (double)w[at] : 1.0;
            g[at] = (T)(m * (am * dh[j + 2] + a0 * dh[j + 1] + ap * dh[j]));
        }
    }
}

bool tt_shape(int nt, int ntr, int K) {
    return nt >= 1 && ntr >= 1 && K >= 1 && gather_blocks(nt, ntr) <= 0x7fffffff && tt_lag_tiles(nt, K) <= 65535;
}

}  // namespace

template <typename T>
hipError_t launch_tt_xcorr(double *part, const T *s, const T *d, const T *w, int K, int nt, int ntr, hipStream_t st) {
    if (!part || !s || !d || !tt_shape(nt, ntr, K)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)gather_xtiles(ntr), (unsigned)tt_lag_tiles(nt, K), (unsigned)tt_slices(nt, ntr, K));
    hipLaunchKernelGGL(tt_xcorr<T>, grid, dim3(GT_BLOCK), 0, st, part, s, d, w, nt, ntr, tt_reach(nt, K),
                       tt_slice_len(nt, ntr, K));
    return hipGetLastError();
}

hipError_t launch_tt_pick(double *coef, int32_t *lag, double *part, const double *tw, double dt, int K, int nt, int ntr,
                          hipStream_t st) {
    if (!coef || !lag || !part || !tt_shape(nt, ntr, K)) return hipErrorInvalidValue;
    const int slices = tt_slices(nt, ntr, K);
    double *jterm = part + (size_t)slices * tt_lags(nt, K) * ntr;
    hipLaunchKernelGGL(tt_pick, dim3((unsigned)((ntr + TT_PBLOCK - 1) / TT_PBLOCK)), dim3(TT_PBLOCK), 0, st, coef, lag,
                       jterm, part, tw, dt, tt_reach(nt, K), slices, ntr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_sum_partials(jterm, ntr, st);
}

template <typename T>
hipError_t launch_tt_source(T *g, const T *d, const T *w, const double *coef, const int32_t *lag, int nt, int ntr,
                            hipStream_t st) {
    if (!g || !d || !coef || !lag || nt < 1 || ntr < 1 || gather_blocks(nt, ntr) > 0x7fffffff || g == d || g == w)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(tt_source<T>, dim3((unsigned)gather_blocks(nt, ntr)), dim3(GT_BLOCK), 0, st, g, d, w, coef, lag,
                       nt, ntr, gather_xtiles(ntr));
    return hipGetLastError();
}

template hipError_t launch_tt_xcorr<float>(double *, const float *, const float *, const float *, int, int, int,
                                           hipStream_t);
template hipError_t launch_tt_xcorr<double>(double *, const double *, const double *, const double *, int, int, int,
                                            hipStream_t);
template hipError_t launch_tt_source<float>(float *, const float *, const float *, const double *, const int32_t *, int,
                                            int, hipStream_t);
template hipError_t launch_tt_source<double>(double *, const double *, const double *, const double *, const int32_t *,
                                             int, int, hipStream_t);

}  // namespace fwi
