// Trace-normalised correlation misfit of (nt, ntr) trace gathers (fwi_corr.h): the per-trace sums a, b, c of a gather
// pair, the coefficients alpha, beta, rho of every trace with the terms of J, and the elementwise adjoint source.  Its
// own object: the step / tile / point / smoothing / regularisation / data / matching / envelope objects keep their
// pinned kernel counts.
//
// The tile is the shared one of fwi_gather_tile.h (lane = trace, 64 traces by 32 times per block of 256 threads, 8
// consecutive times per thread).  What is new here is a reduction per TRACE: a thread adds its 8 times in ascending
// order, the block adds its four waves per lane in wave order through LDS and writes three doubles per trace and time
// tile; one thread per trace then adds the tiles in ascending order.  No atomics: equal inputs give equal bits.  All
// arithmetic between the loads and the one rounding of g to T is fp64.
#include <hip/hip_runtime.h>

#include "fwi_corr.h"
#include "fwi_gather_tile.h"
#include "fwi_kernels.h"

namespace fwi {

namespace {

static_assert(GT_TT == 32, "corr_tiles (fwi_corr.h) counts tiles of 32 times");
constexpr int CORR_WAVES = GT_BLOCK / GT_LANES;
constexpr int CORR_CBLOCK = 256;

template <typename T>
__global__ __launch_bounds__(GT_BLOCK) void corr_sums(double *part, const T *s, const T *d, const T *w, int nt, int ntr,
                                                      int xtiles) {
    __shared__ double sums[3][CORR_WAVES][GT_LANES];
    const GatherTile c = gather_tile(xtiles);
    double a = 0.0, b = 0.0, cc = 0.0;
    if (c.gx < ntr) {
#pragma unroll
        for (int j = 0; j < GT_TO; ++j) {
            if (c.tn0 + j < nt) {
                const int64_t at = (int64_t)(c.tn0 + j) * ntr + c.gx;
                const double m = w ? (double)w[at] : 1.0;
                const double sv = m * (double)s[at], dv = m * (double)d[at];
                a = fma(sv, sv, a);
                b = fma(dv, dv, b);
                cc = fma(sv, dv, cc);
            }
        }
    }
    sums[0][c.grp][c.lane] = a;
    sums[1][c.grp][c.lane] = b;
    sums[2][c.grp][c.lane] = cc;
    __syncthreads();
    // wave q adds the four waves' sums of quantity q, per lane, in wave order
    if (c.grp < 3 && c.gx < ntr) {
        double v = sums[c.grp][0][c.lane];
#pragma unroll
        for (int g = 1; g < CORR_WAVES; ++g) v += sums[c.grp][g][c.lane];
        const int64_t tile = blockIdx.x / xtiles;
        part[(3 * tile + c.grp) * ntr + c.gx] = v;
    }
}

__global__ __launch_bounds__(CORR_CBLOCK) void corr_coeffs(double *coef, double *jterm, const double *part,
                                                           const double *tw, double eps2, int tiles, int ntr) {
    const int j = blockIdx.x * CORR_CBLOCK + threadIdx.x;
    if (j >= ntr) return;
    double a = 0.0, b = 0.0, c = 0.0;
    for (int64_t t = 0; t < tiles; ++t) {
        a += part[(3 * t + 0) * ntr + j];
        b += part[(3 * t + 1) * ntr + j];
        c += part[(3 * t + 2) * ntr + j];
    }
    const double as = a + eps2, bs = b + eps2, wj = tw ? tw[j] : 1.0;
    double alpha = 0.0, beta = 0.0, rho = 0.0, term = 0.0;
    if (b > 0.0 && as > 0.0) {  // the trace counts
        const double nn = sqrt(as) * sqrt(bs);
        rho = c / nn;
        alpha = -wj / nn;
        beta = c / as;
        term = wj * (1.0 - rho);
    }
    coef[j] = alpha;
    coef[(int64_t)ntr + j] = beta;
    coef[2 * (int64_t)ntr + j] = rho;
    jterm[j] = term;
}

template <typename T>
__global__ __launch_bounds__(GT_BLOCK) void corr_source(T *g, const T *s, const T *d, const T *w, const double *coef,
                                                        int nt, int ntr, int xtiles) {
    const GatherTile c = gather_tile(xtiles);
    if (c.gx >= ntr) return;
    const double alpha = coef[c.gx], beta = coef[(int64_t)ntr + c.gx];
#pragma unroll
    for (int j = 0; j < GT_TO; ++j) {
        if (c.tn0 + j < nt) {
            const int64_t at = (int64_t)(c.tn0 + j) * ntr + c.gx;
            const double m = w ? (double)w[at] : 1.0;
            const double sv = m * (double)s[at], dv = m * (double)d[at];
            g[at] = (T)(m * (alpha * (dv - beta * sv)));
        }
    }
}

bool corr_shape(int nt, int ntr) { return nt >= 1 && ntr >= 1 && gather_blocks(nt, ntr) <= 0x7fffffff; }

}  // namespace

template <typename T>
hipError_t launch_corr_sums(double *part, const T *s, const T *d, const T *w, int nt, int ntr, hipStream_t st) {
    if (!part || !s || !d || !corr_shape(nt, ntr)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(corr_sums<T>, dim3((unsigned)gather_blocks(nt, ntr)), dim3(GT_BLOCK), 0, st, part, s, d, w, nt,
                       ntr, gather_xtiles(ntr));
    return hipGetLastError();
}

hipError_t launch_corr_coeffs(double *coef, double *part, const double *tw, double eps, int nt, int ntr, hipStream_t st) {
    if (!coef || !part || !corr_shape(nt, ntr) || !(eps >= 0.0)) return hipErrorInvalidValue;
    const int tiles = corr_tiles(nt);
    double *jterm = part + (size_t)3 * tiles * ntr;
    hipLaunchKernelGGL(corr_coeffs, dim3((unsigned)((ntr + CORR_CBLOCK - 1) / CORR_CBLOCK)), dim3(CORR_CBLOCK), 0, st,
                       coef, jterm, part, tw, eps * eps, tiles, ntr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_sum_partials(jterm, ntr, st);
}

template <typename T>
hipError_t launch_corr_source(T *g, const T *s, const T *d, const T *w, const double *coef, int nt, int ntr,
                              hipStream_t st) {
    if (!g || !s || !d || !coef || !corr_shape(nt, ntr) || g == w) return hipErrorInvalidValue;
    hipLaunchKernelGGL(corr_source<T>, dim3((unsigned)gather_blocks(nt, ntr)), dim3(GT_BLOCK), 0, st, g, s, d, w, coef,
                       nt, ntr, gather_xtiles(ntr));
    return hipGetLastError();
}

template hipError_t launch_corr_sums<float>(double *, const float *, const float *, const float *, int, int, hipStream_t);
template hipError_t launch_corr_sums<double>(double *, const double *, const double *, const double *, int, int,
                                             hipStream_t);
template hipError_t launch_corr_source<float>(float *, const float *, const float *, const float *, const double *, int,
                                              int, hipStream_t);
template hipError_t launch_corr_source<double>(double *, const double *, const double *, const double *, const double *,
                                               int, int, hipStream_t);

}  // namespace fwi
