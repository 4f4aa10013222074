// Envelope misfit of (nt, ntr) trace gathers (fwi_envelope.h): the antisymmetric Hilbert FIR filter H along time, the
// envelopes E(s), E(d) of two gathers, the residual e of their p-th powers with its fixed-order sum of squares, and the
// adjoint source q = g1 - H g2.  Its own object: the step / tile / point / smoothing / regularisation / data / matching
// objects keep their pinned kernel counts.
//
// The tile, the march of the input rows through LDS, the odd-taps-only split and the fixed-order sums are the shared
// ones of fwi_gather_tile.h.  The forward kernel marches s and d together (16 accumulators: H s and H d) in chunks of
// ENV_CH = 16 rows (16 KiB); the taps h_1 .. h_Q sit in LDS behind them (at most 4096 doubles, 32 KiB): 48 KiB at most,
// below the 64 KiB a block gets without an opt-in attribute.  g1, g2 and q are each rounded to T once, when they are
// stored.  The squares of the unrounded e are what the thread sums.
#include <hip/hip_runtime.h>

#include "fwi_data.h"
#include "fwi_envelope.h"
#include "fwi_gather_tile.h"
#include "fwi_kernels.h"

namespace fwi {

namespace {

constexpr int ENV_CH = 16;
static_assert((2 * ENV_CH * GT_LANES + FIR_RMAX) * sizeof(double) <= 64 * 1024, "no opt-in for dynamic LDS");

struct EnvArgs {
    int nt, ntr, Q, xtiles;
    int odd_only;  // every even tap is zero: their products are not formed
    int power;     // 1 or 2
    double eps2;   // eps^2
};

// the taps h_1 .. h_Q into LDS behind the NS signals' rows
template <int NS>
__device__ __forceinline__ AntisymmetricTaps env_taps(double *smem, const double *h, const EnvArgs &a) {
    double *sH = smem + NS * ENV_CH * GT_LANES;
    for (int k = threadIdx.x; k < a.Q; k += GT_BLOCK) sH[k] = h[k];
    return AntisymmetricTaps{sH, a.Q, a.odd_only != 0};
}

template <typename T>
__global__ __launch_bounds__(GT_BLOCK) void env_forward(T *g1, T *g2, const T *s, const T *d, const T *w,
                                                        const double *h, EnvArgs a, double *partial) {
    extern __shared__ double smem[];
    const GatherTile c = gather_tile(a.xtiles);
    double acc[2][GT_TO];  // H s, H d
    gather_march<2, ENV_CH>(acc, smem, c, a.nt, a.ntr,
                            [&](int sig, int64_t at) { return (double)(sig ? d[at] : s[at]); }, env_taps<2>(smem, h, a));

    double sq = 0.0;
    if (c.gx < a.ntr) {
#pragma unroll
        for (int j = 0; j < GT_TO; ++j) {
            if (c.tn0 + j < a.nt) {
                const int64_t at = (int64_t)(c.tn0 + j) * a.ntr + c.gx;
                const double sv = (double)s[at], dv = (double)d[at], hs = acc[0][j], hd = acc[1][j];
                const double es2 = fma(sv, sv, fma(hs, hs, a.eps2)), ed2 = fma(dv, dv, fma(hd, hd, a.eps2));
                const double m = w ? (double)w[at] : 1.0;
                double e, cf;
                if (a.power == 1) {
                    const double es = sqrt(es2);
                    e = m * (es - sqrt(ed2));
                    cf = m * e / es;  // (eps > 0: es > 0)
                } else {
                    e = m * (es2 - ed2);
                    cf = 2.0 * (m * e);
                }
                g1[at] = (T)(cf * sv);
                g2[at] = (T)(cf * hs);
                sq += e * e;
            }
        }
    }
    __syncthreads();  // the last chunk is used up: its LDS takes the block's sum
    block_tree_sum_to_partial(sq, smem, partial);
}

template <typename T>
__global__ __launch_bounds__(GT_BLOCK) void env_adjoint(T *q, const T *g1, const T *g2, const double *h, EnvArgs a) {
    extern __shared__ double smem[];
    const GatherTile c = gather_tile(a.xtiles);
    double acc[1][GT_TO];  // H g2
    gather_march<1, ENV_CH>(acc, smem, c, a.nt, a.ntr, [&](int, int64_t at) { return (double)g2[at]; },
                            env_taps<1>(smem, h, a));
    if (c.gx >= a.ntr) return;
#pragma unroll
    for (int j = 0; j < GT_TO; ++j) {
        if (c.tn0 + j < a.nt) {
            const int64_t at = (int64_t)(c.tn0 + j) * a.ntr + c.gx;
            q[at] = (T)((double)g1[at] - acc[0][j]);
        }
    }
}

bool env_args(EnvArgs *a, int Q, bool odd_only, int nt, int ntr) {
    if (nt < 1 || ntr < 1 || Q < 1 || Q > FIR_RMAX || gather_blocks(nt, ntr) > 0x7fffffff) return false;
    a->nt = nt, a->ntr = ntr, a->xtiles = gather_xtiles(ntr);
    a->Q = Q < nt - 1 ? Q : nt - 1;  // the taps beyond nt - 1 meet no sample
    a->odd_only = odd_only ? 1 : 0;
    a->power = 0, a->eps2 = 0.0;
    return true;
}

}  // namespace

template <typename T>
hipError_t launch_env_forward(T *g1, T *g2, const T *s, const T *d, const T *w, const double *h, int Q, bool odd_only,
                              int power, double eps, int nt, int ntr, double *partial, hipStream_t st) {
    EnvArgs a;
    if (!g1 || !g2 || !s || !d || !h || !partial || !env_args(&a, Q, odd_only, nt, ntr) || (power != 1 && power != 2) ||
        !(eps >= 0.0) || (power == 1 && !(eps > 0.0)) || g1 == g2 || g1 == s || g1 == d || g1 == w || g2 == s ||
        g2 == d || g2 == w)
        return hipErrorInvalidValue;
    a.power = power, a.eps2 = eps * eps;
    const int64_t blocks = gather_blocks(nt, ntr);
    const size_t lds = (size_t)(2 * ENV_CH * GT_LANES + a.Q) * sizeof(double);
    hipLaunchKernelGGL(env_forward<T>, dim3((unsigned)blocks), dim3(GT_BLOCK), lds, st, g1, g2, s, d, w, h, a, partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_sum_partials(partial, blocks, st);
}

template <typename T>
hipError_t launch_env_adjoint(T *q, const T *g1, const T *g2, const double *h, int Q, bool odd_only, int nt, int ntr,
                              hipStream_t st) {
    EnvArgs a;
    if (!q || !g1 || !g2 || !h || !env_args(&a, Q, odd_only, nt, ntr) || q == g2) return hipErrorInvalidValue;
    const size_t lds = (size_t)(ENV_CH * GT_LANES + a.Q) * sizeof(double);
    hipLaunchKernelGGL(env_adjoint<T>, dim3((unsigned)gather_blocks(nt, ntr)), dim3(GT_BLOCK), lds, st, q, g1, g2, h, a);
    return hipGetLastError();
}

template hipError_t launch_env_forward<float>(float *, float *, const float *, const float *, const float *,
                                              const double *, int, bool, int, double, int, int, double *, hipStream_t);
template hipError_t launch_env_forward<double>(double *, double *, const double *, const double *, const double *,
                                               const double *, int, bool, int, double, int, int, double *, hipStream_t);
template hipError_t launch_env_adjoint<float>(float *, const float *, const float *, const double *, int, bool, int, int,
                                              hipStream_t);
template hipError_t launch_env_adjoint<double>(double *, const double *, const double *, const double *, int, bool, int,
                                               int, hipStream_t);

}  // namespace fwi
