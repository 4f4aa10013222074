// Envelope misfit of (nt, ntr) trace gathers (fwi_envelope.h): the antisymmetric Hilbert FIR filter H along time, the
// envelopes E(s), E(d) of two gathers, the residual e of their p-th powers with its fixed-order sum of squares, and the
// adjoint source q = g1 - H g2.  Its own object: the step / tile / point / smoothing / regularisation / data / matching
// objects keep their pinned kernel counts.
//
// Layout and discipline are fir_time's (fwi_data.hip).  Lane = trace: every global load and store runs along the fast
// axis.  A block of 256 threads owns FIR_LANES = 64 traces by FIR_TT = 32 output times; each of its four waves keeps
// FIR_TO = 8 consecutive output times per lane in registers, of H s AND H d in the forward kernel (16 accumulators).
// The taps h_1 .. h_Q sit in LDS (at most 4096 doubles, 32 KiB).  The input rows t0 - Q .. t0 + FIR_TT + Q - 1 pass
// through LDS in chunks of ENV_CH = 16 rows, in ascending time, both signals of the forward kernel together (16 KiB):
// 48 KiB at most, below the 64 KiB a block gets without an opt-in attribute.  Per chunk
//   stage   the chunk's rows as fp64; rows outside [0, nt) and traces >= ntr are not read, their slots hold zeros;
//   sum     per 8 rows: the 15 coefficients w(kappa) = -sign(kappa) h_|kappa|, kappa = row - output, that 8 rows and 8
//           outputs can pair (zero where kappa = 0 or |kappa| > Q) go to registers, then every row's x is read once
//           from LDS (lane-contiguous doubles: no bank conflict) and added into the accumulators.
// A Hilbert transformer's even taps are zero.  Where the caller says so (odd_only), a group forms only the products whose
// kappa is odd: which those are depends on the parity of the group's first kappa alone, which is the same for a whole
// wave, so the branch is uniform and each side is straight-line code of half the FMAs.  The products left out are
// 0 * x, which add nothing to a finite sum: the bits do not depend on it.
// For every output the terms are added over ascending row time, in fp64; g1, g2 and q are each rounded to T once, when
// they are stored.  The squares of the unrounded e are summed per thread over ascending time, over the block by a fixed
// tree into partial[block]; env_sum adds the partials in a fixed order.  No atomics.
#include <hip/hip_runtime.h>

#include "fwi_data.h"
#include "fwi_envelope.h"

namespace fwi {

namespace {

constexpr int ENV_BLOCK = 256, ENV_CH = 16;
static_assert(ENV_BLOCK == 64 * (FIR_TT / FIR_TO) && FIR_LANES == 64, "one wave per FIR_TO output times");
static_assert(ENV_CH % FIR_TO == 0 && ENV_CH * FIR_LANES >= ENV_BLOCK, "whole groups of rows; room for the block's sum");
static_assert((2 * ENV_CH * FIR_LANES + FIR_RMAX) * sizeof(double) <= 64 * 1024, "no opt-in for dynamic LDS");

struct EnvArgs {
    int nt, ntr, Q, xtiles;
    int odd_only;  // every even tap is zero: their products are not formed
    int power;     // 1 or 2
    double eps2;   // eps^2
};

// one group of FIR_TO rows (sX points at the first one's slot of this lane, the signals ENV_CH rows apart) against the
// thread's FIR_TO outputs; d0 = kappa of (row 0, output 0).  PAR < 0: every product; otherwise PAR = d0 & 1 and only
// the products with odd kappa = d0 + i - j.
template <int NS, int PAR>
__device__ __forceinline__ void env_group(double (&acc)[NS][FIR_TO], const double *sX, const double *sH, int d0, int Q) {
    double w[2 * FIR_TO - 1];
#pragma unroll
    for (int q = 0; q < 2 * FIR_TO - 1; ++q) {
        if (PAR >= 0 && ((PAR + q) & 1)) continue;  // kappa = d0 + q - 7 is even
        const int k = d0 + q - (FIR_TO - 1), kk = k < 0 ? -k : k;
        const double hv = (kk >= 1 && kk <= Q) ? sH[kk - 1] : 0.0;
        w[q] = k < 0 ? hv : -hv;  // x[n - k] enters with +h_k, x[n + k] with -h_k
    }
#pragma unroll
    for (int i = 0; i < FIR_TO; ++i) {
        double xv[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) xv[s] = sX[(s * ENV_CH + i) * FIR_LANES];
#pragma unroll
        for (int j = 0; j < FIR_TO; ++j) {
            const int q = i - j + FIR_TO - 1;
            if (PAR >= 0 && ((PAR + q) & 1)) continue;
#pragma unroll
            for (int s = 0; s < NS; ++s) acc[s][j] = fma(w[q], xv[s], acc[s][j]);
        }
    }
}

// acc[s][j] := (H in_s)[tn0 + j, gx] for the NS signals; smem: NS * ENV_CH * FIR_LANES doubles of rows, then Q taps
template <typename T, int NS>
__device__ __forceinline__ void env_hilbert(double (&acc)[NS][FIR_TO], const T *in0, const T *in1, const double *h,
                                            const EnvArgs &a, double *smem, int x0, int t0) {
    double *sX = smem;                            // [NS][ENV_CH][FIR_LANES]
    double *sH = smem + NS * ENV_CH * FIR_LANES;  // [Q]: h_1 .. h_Q
    const int tid = threadIdx.x, lane = tid & 63, grp = tid >> 6;
    const int tn0 = t0 + grp * FIR_TO;  // this thread's first output time
    const int Q = a.Q;
    for (int k = tid; k < Q; k += ENV_BLOCK) sH[k] = h[k];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int j = 0; j < FIR_TO; ++j) acc[s][j] = 0.0;

    const int lo = t0 - Q > 0 ? t0 - Q : 0, hi = t0 + FIR_TT + Q < a.nt ? t0 + FIR_TT + Q : a.nt;
    for (int m0 = lo; m0 < hi; m0 += ENV_CH) {
        __syncthreads();  // the chunk before is used up
        for (int i = tid; i < ENV_CH * FIR_LANES; i += ENV_BLOCK) {
            const int gm = m0 + (i >> 6), g = x0 + (i & 63);
            double v0 = 0.0, v1 = 0.0;
            if (gm < hi && g < a.ntr) {
                const int64_t at = (int64_t)gm * a.ntr + g;
                v0 = (double)in0[at];
                if (NS > 1) v1 = (double)in1[at];
            }
            sX[i] = v0;
            if (NS > 1) sX[ENV_CH * FIR_LANES + i] = v1;
        }
        __syncthreads();
#pragma unroll 1
        for (int mb = 0; mb < ENV_CH; mb += FIR_TO) {
            const int d0 = m0 + mb - tn0;  // the group pairs kappa in d0 - 7 .. d0 + 7
            if (m0 + mb >= hi || d0 + (FIR_TO - 1) < -Q || d0 - (FIR_TO - 1) > Q) continue;  // (the same for a whole wave)
            const double *row = sX + mb * FIR_LANES + lane;
            if (!a.odd_only)
                env_group<NS, -1>(acc, row, sH, d0, Q);
            else if (d0 & 1)
                env_group<NS, 1>(acc, row, sH, d0, Q);
            else
                env_group<NS, 0>(acc, row, sH, d0, Q);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(ENV_BLOCK) void env_forward(T *g1, T *g2, const T *s, const T *d, const T *w,
                                                         const double *h, EnvArgs a, double *partial) {
    extern __shared__ double smem[];
    const int tid = threadIdx.x, lane = tid & 63, grp = tid >> 6;
    const int x0 = (int)(blockIdx.x % a.xtiles) * FIR_LANES, t0 = (int)(blockIdx.x / a.xtiles) * FIR_TT;
    const int gx = x0 + lane, tn0 = t0 + grp * FIR_TO;
    double acc[2][FIR_TO];  // H s, H d
    env_hilbert<T, 2>(acc, s, d, h, a, smem, x0, t0);

    double sq = 0.0;
    if (gx < a.ntr) {
#pragma unroll
        for (int j = 0; j < FIR_TO; ++j) {
            if (tn0 + j < a.nt) {
                const int64_t at = (int64_t)(tn0 + j) * a.ntr + gx;
                const double sv = (double)s[at], dv = (double)d[at], hs = acc[0][j], hd = acc[1][j];
                const double es2 = fma(sv, sv, fma(hs, hs, a.eps2)), ed2 = fma(dv, dv, fma(hd, hd, a.eps2));
                const double m = w ? (double)w[at] : 1.0;
                double e, c;
                if (a.power == 1) {
                    const double es = sqrt(es2);
                    e = m * (es - sqrt(ed2));
                    c = m * e / es;  // (eps > 0: es > 0)
                } else {
                    e = m * (es2 - ed2);
                    c = 2.0 * (m * e);
                }
                g1[at] = (T)(c * sv);
                g2[at] = (T)(c * hs);
                sq += e * e;
            }
        }
    }
    __syncthreads();  // the last chunk is used up: its LDS takes the block's sum
    smem[tid] = sq;
    __syncthreads();
    for (int st = ENV_BLOCK / 2; st > 0; st >>= 1) {
        if (tid < st) smem[tid] += smem[tid + st];
        __syncthreads();
    }
    if (tid == 0) partial[blockIdx.x] = smem[0];
}

template <typename T>
__global__ __launch_bounds__(ENV_BLOCK) void env_adjoint(T *q, const T *g1, const T *g2, const double *h, EnvArgs a) {
    extern __shared__ double smem[];
    const int tid = threadIdx.x, lane = tid & 63, grp = tid >> 6;
    const int x0 = (int)(blockIdx.x % a.xtiles) * FIR_LANES, t0 = (int)(blockIdx.x / a.xtiles) * FIR_TT;
    const int gx = x0 + lane, tn0 = t0 + grp * FIR_TO;
    double acc[1][FIR_TO];  // H g2
    env_hilbert<T, 1>(acc, g2, nullptr, h, a, smem, x0, t0);
    if (gx >= a.ntr) return;
#pragma unroll
    for (int j = 0; j < FIR_TO; ++j) {
        if (tn0 + j < a.nt) {
            const int64_t at = (int64_t)(tn0 + j) * a.ntr + gx;
            q[at] = (T)((double)g1[at] - acc[0][j]);
        }
    }
}

// partial[n] = sum of partial[0 .. n): strided per thread, then a fixed tree
__global__ __launch_bounds__(ENV_BLOCK) void env_sum(double *partial, int64_t n) {
    __shared__ double sRed[ENV_BLOCK];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int64_t i = tid; i < n; i += ENV_BLOCK) acc += partial[i];
    sRed[tid] = acc;
    __syncthreads();
    for (int s = ENV_BLOCK / 2; s > 0; s >>= 1) {
        if (tid < s) sRed[tid] += sRed[tid + s];
        __syncthreads();
    }
    if (tid == 0) partial[n] = sRed[0];
}

bool env_args(EnvArgs *a, int Q, bool odd_only, int nt, int ntr) {
    if (nt < 1 || ntr < 1 || Q < 1 || Q > FIR_RMAX || env_blocks(nt, ntr) > 0x7fffffff) return false;
    a->nt = nt, a->ntr = ntr, a->xtiles = (ntr + FIR_LANES - 1) / FIR_LANES;
    a->Q = Q < nt - 1 ? Q : nt - 1;  // the taps beyond nt - 1 meet no sample
    a->odd_only = odd_only ? 1 : 0;
    a->power = 0, a->eps2 = 0.0;
    return true;
}

}  // namespace

int64_t env_blocks(int nt, int ntr) {
    return (int64_t)((ntr + FIR_LANES - 1) / FIR_LANES) * ((nt + FIR_TT - 1) / FIR_TT);
}

template <typename T>
hipError_t launch_env_forward(T *g1, T *g2, const T *s, const T *d, const T *w, const double *h, int Q, bool odd_only,
                              int power, double eps, int nt, int ntr, double *partial, hipStream_t st) {
    EnvArgs a;
    if (!g1 || !g2 || !s || !d || !h || !partial || !env_args(&a, Q, odd_only, nt, ntr) || (power != 1 && power != 2) ||
        !(eps >= 0.0) || (power == 1 && !(eps > 0.0)) || g1 == g2 || g1 == s || g1 == d || g1 == w || g2 == s ||
        g2 == d || g2 == w)
        return hipErrorInvalidValue;
    a.power = power, a.eps2 = eps * eps;
    const int64_t blocks = env_blocks(nt, ntr);
    const size_t lds = (size_t)(2 * ENV_CH * FIR_LANES + a.Q) * sizeof(double);
    hipLaunchKernelGGL(env_forward<T>, dim3((unsigned)blocks), dim3(ENV_BLOCK), lds, st, g1, g2, s, d, w, h, a, partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(env_sum, dim3(1), dim3(ENV_BLOCK), 0, st, partial, blocks);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_env_adjoint(T *q, const T *g1, const T *g2, const double *h, int Q, bool odd_only, int nt, int ntr,
                              hipStream_t st) {
    EnvArgs a;
    if (!q || !g1 || !g2 || !h || !env_args(&a, Q, odd_only, nt, ntr) || q == g2) return hipErrorInvalidValue;
    const size_t lds = (size_t)(ENV_CH * FIR_LANES + a.Q) * sizeof(double);
    hipLaunchKernelGGL(env_adjoint<T>, dim3((unsigned)env_blocks(nt, ntr)), dim3(ENV_BLOCK), lds, st, q, g1, g2, h, a);
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
