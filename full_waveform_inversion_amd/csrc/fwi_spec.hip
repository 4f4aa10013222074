// Frequency-domain (spectral) data misfit of (nt, ntr) trace gathers (fwi_spec.h): the Fourier coefficients S, O of a
// gather pair at F frequencies per time segment, the misfit and its derivative G per (frequency, trace) pair with the
// terms of J, and the adjoint source.  Its own object: the step / tile / point / smoothing / regularisation / data /
// matching / envelope / correlation / traveltime / transport objects keep their pinned kernel counts.
//
// Lane = trace, time the slow axis, as in fwi_gather_tile.h.  The analysis owns 64 traces by SPEC_SEG = 256 times per
// block of 1024 threads: each of its 16 waves keeps 16 consecutive times of both weighted gathers per lane in registers
// and walks the frequencies one at a time (a second frequency's twiddles in flight spill scalar
// registers).  The twiddles of a wave's rows at one frequency are contiguous in the frequency-major table and their
// address is the same in every lane: they come through the scalar data cache and take no vector register.  A thread adds
// its times by fma in ascending order, the block adds its waves per lane in wave order through LDS, the coefficient
// kernel adds the segments in ascending order and launch_sum_partials the terms of J in its fixed order.  No atomics:
// equal inputs give equal bits.  All arithmetic between the loads and the one rounding of g to T is fp64.
#include <hip/hip_runtime.h>

#include "fwi_gather_tile.h"
#include "fwi_kernels.h"
#include "fwi_spec.h"

namespace fwi {

namespace {

constexpr int SPEC_BLOCK = 1024, SPEC_WAVES = SPEC_BLOCK / GT_LANES, SPEC_TO = SPEC_SEG / SPEC_WAVES;
constexpr int SPEC_CBLOCK = 256;
static_assert(SPEC_WAVES * SPEC_TO == SPEC_SEG && SPEC_TO % GT_TO == 0 && SPEC_SEG % GT_TT == 0,
              "whole groups of 8 rows per wave; the source's tiles end on rows the table holds");

template <typename T>
__global__ __launch_bounds__(SPEC_BLOCK) void spec_analysis(double *__restrict__ part, const T *__restrict__ s,
                                                            const T *__restrict__ d, const T *__restrict__ w,
                                                            const double *__restrict__ table, int F, int nt, int ntr,
                                                            int xtiles, int rows) {
    __shared__ double sums[4][SPEC_WAVES][GT_LANES];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int seg = blockIdx.x / xtiles, gx = (int)(blockIdx.x % xtiles) * GT_LANES + lane;
    const int r0 = seg * SPEC_SEG + wave * SPEC_TO;  // this wave's first row: the same in every lane
    double sv[SPEC_TO], dv[SPEC_TO];
#pragma unroll
    for (int i = 0; i < SPEC_TO; ++i) {
        sv[i] = dv[i] = 0.0;
        if (gx < ntr && r0 + i < nt) {
            const int64_t at = (int64_t)(r0 + i) * ntr + gx;
            const double m = w ? (double)w[at] : 1.0;
            sv[i] = m * (double)s[at];
            dv[i] = m * (double)d[at];
        }
    }
#pragma unroll 1
    for (int k = 0; k < F; ++k) {
        const double *t = table + ((int64_t)k * rows + r0) * 2;  // (cos, sin) of rows r0 .. r0 + 15: 256 contiguous bytes
        double sc = 0.0, ss = 0.0, dc = 0.0, ds = 0.0;
#pragma unroll
        for (int i = 0; i < SPEC_TO; ++i) {
            const double c = t[2 * i], sn = t[2 * i + 1];
            sc = fma(sv[i], c, sc);
            ss = fma(sv[i], sn, ss);
            dc = fma(dv[i], c, dc);
            ds = fma(dv[i], sn, ds);
        }
        sums[0][wave][lane] = sc;
        sums[1][wave][lane] = -ss;
        sums[2][wave][lane] = dc;
        sums[3][wave][lane] = -ds;
        __syncthreads();
        // wave q adds the 16 waves' sums of quantity q, per lane, in wave order
        if (wave < 4 && gx < ntr) {
            double v = sums[wave][0][lane];
#pragma unroll
            for (int g = 1; g < SPEC_WAVES; ++g) v += sums[wave][g][lane];
            part[(((int64_t)seg * F + k) * 4 + wave) * ntr + gx] = v;
        }
        __syncthreads();  // the sums are used up before the next frequency's are written
    }
}

// Im(S conj O) = S_i O_r - S_r O_i from two rounded products, never a fused one: equal S and O then give exactly 0
__device__ __forceinline__ double cross_im(double sr, double si, double orr, double oi) {
#pragma clang fp contract(off)
    const double p = si * orr;
    const double q = sr * oi;
    return p - q;
}

__global__ __launch_bounds__(SPEC_CBLOCK) void spec_coeffs(double *__restrict__ coef, uint8_t *__restrict__ counts,
                                                           const double *__restrict__ part, const double *__restrict__ fw,
                                                           const double *__restrict__ tw, int kind, double eps2, int F,
                                                           int segs, int ntr) {
    const int64_t p = (int64_t)blockIdx.x * SPEC_CBLOCK + threadIdx.x, npair = (int64_t)F * ntr;
    if (p >= npair) return;
    const int k = (int)(p / ntr), j = (int)(p % ntr);
    double sr = 0.0, si = 0.0, orr = 0.0, oi = 0.0;
    for (int64_t g = 0; g < segs; ++g) {
        const double *q = part + ((g * F + k) * 4) * ntr + j;
        sr += q[0];
        si += q[ntr];
        orr += q[2 * (int64_t)ntr];
        oi += q[3 * (int64_t)ntr];
    }
    const double wkj = (fw ? fw[k] : 1.0) * (tw ? tw[j] : 1.0);
    const double s2 = sr * sr + si * si, o2 = orr * orr + oi * oi;
    const bool both = s2 > eps2 && o2 > eps2;  // the counting rule of PHASE and LOG
    const bool amp = kind == SPEC_LOGAMP || (kind == SPEC_LOG && both), ph = (kind == SPEC_PHASE || kind == SPEC_LOG) && both;
    double gr = 0.0, gi = 0.0, term = 0.0, a = 0.0, phi = 0.0;
    if (amp || both) a = 0.5 * log((s2 + eps2) / (o2 + eps2));
    if (both) phi = atan2(cross_im(sr, si, orr, oi), sr * orr + si * oi);
    if (kind == SPEC_L2) {
        const double dr = sr - orr, di = si - oi;
        gr = wkj * dr, gi = wkj * di;
        term = 0.5 * wkj * (dr * dr + di * di);
    }
    if (amp) {
        const double c = wkj * a / (s2 + eps2);
        gr += c * sr, gi += c * si;
        term += 0.5 * wkj * a * a;
    }
    if (ph) {  // i S = -S_i + i S_r
        const double c = wkj * phi / s2;
        gr -= c * si, gi += c * sr;
        term += 0.5 * wkj * phi * phi;
    }
    coef[p] = gr;
    coef[npair + p] = gi;
    coef[2 * npair + p] = phi;
    coef[3 * npair + p] = a;
    coef[4 * npair + p] = term;
    counts[p] = (kind == SPEC_L2 || kind == SPEC_LOGAMP || both) ? 1 : 0;
}

template <typename T>
__global__ __launch_bounds__(GT_BLOCK) void spec_source(T *__restrict__ g, const T *__restrict__ w,
                                                        const double *__restrict__ coef, const double *__restrict__ table,
                                                        int F, int nt, int ntr, int xtiles, int rows) {
    const int lane = threadIdx.x & 63, grp = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int gx = (int)(blockIdx.x % xtiles) * GT_LANES + lane;
    const int tn0 = (int)(blockIdx.x / xtiles) * GT_TT + grp * GT_TO;  // this wave's first row: the same in every lane
    if (gx >= ntr) return;
    const int64_t npair = (int64_t)F * ntr;
    double acc[GT_TO];
#pragma unroll
    for (int i = 0; i < GT_TO; ++i) acc[i] = 0.0;
#pragma unroll 1
    for (int k = 0; k < F; ++k) {
        const double *t = table + ((int64_t)k * rows + tn0) * 2;  // (cos, sin) of rows tn0 .. tn0 + 7: 128 contiguous bytes
        const double gr = coef[(int64_t)k * ntr + gx], ngi = -coef[npair + (int64_t)k * ntr + gx];
#pragma unroll
        for (int i = 0; i < GT_TO; ++i) {
            acc[i] = fma(gr, t[2 * i], acc[i]);
            acc[i] = fma(ngi, t[2 * i + 1], acc[i]);
        }
    }
#pragma unroll
    for (int i = 0; i < GT_TO; ++i) {
        if (tn0 + i < nt) {
            const int64_t at = (int64_t)(tn0 + i) * ntr + gx;
            g[at] = (T)((w ? (double)w[at] : 1.0) * acc[i]);
        }
    }
}

bool spec_shape(int F, int nt, int ntr) {
    return F >= 1 && nt >= 1 && ntr >= 1 && gather_blocks(nt, ntr) <= 0x7fffffff && (int64_t)F * ntr <= 0x7fffffff;
}

}  // namespace

template <typename T>
hipError_t launch_spec_analysis(double *part, const T *s, const T *d, const T *w, const double *table, int F, int nt,
                                int ntr, hipStream_t st) {
    if (!part || !s || !d || !table || !spec_shape(F, nt, ntr)) return hipErrorInvalidValue;
    const int xtiles = gather_xtiles(ntr);
    hipLaunchKernelGGL(spec_analysis<T>, dim3((unsigned)((int64_t)xtiles * spec_segments(nt))), dim3(SPEC_BLOCK), 0, st,
                       part, s, d, w, table, F, nt, ntr, xtiles, spec_table_rows(nt));
    return hipGetLastError();
}

hipError_t launch_spec_coeffs(double *coef, uint8_t *counts, const double *part, const double *fw, const double *tw,
                              int kind, double eps, int F, int nt, int ntr, hipStream_t st) {
    if (!coef || !counts || !part || !spec_shape(F, nt, ntr) || !(eps >= 0.0) || kind < SPEC_L2 || kind > SPEC_LOG)
        return hipErrorInvalidValue;
    const int64_t npair = (int64_t)F * ntr;
    hipLaunchKernelGGL(spec_coeffs, dim3((unsigned)((npair + SPEC_CBLOCK - 1) / SPEC_CBLOCK)), dim3(SPEC_CBLOCK), 0, st,
                       coef, counts, part, fw, tw, kind, eps * eps, F, spec_segments(nt), ntr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_sum_partials(coef + 4 * npair, npair, st);
}

template <typename T>
hipError_t launch_spec_source(T *g, const T *w, const double *coef, const double *table, int F, int nt, int ntr,
                              hipStream_t st) {
    if (!g || !coef || !table || !spec_shape(F, nt, ntr) || g == w) return hipErrorInvalidValue;
    hipLaunchKernelGGL(spec_source<T>, dim3((unsigned)gather_blocks(nt, ntr)), dim3(GT_BLOCK), 0, st, g, w, coef, table,
                       F, nt, ntr, gather_xtiles(ntr), spec_table_rows(nt));
    return hipGetLastError();
}

template hipError_t launch_spec_analysis<float>(double *, const float *, const float *, const float *, const double *, int,
                                                int, int, hipStream_t);
template hipError_t launch_spec_analysis<double>(double *, const double *, const double *, const double *, const double *,
                                                 int, int, int, hipStream_t);
template hipError_t launch_spec_source<float>(float *, const float *, const double *, const double *, int, int, int,
                                              hipStream_t);
template hipError_t launch_spec_source<double>(double *, const double *, const double *, const double *, int, int, int,
                                               hipStream_t);

}  // namespace fwi
