// Symmetric FIR filtering along time of (nt, ntr) trace gathers, with optional per-sample weights before and after the
// filter and a reproducible sum of squares (fwi_data.h).  Its own object: the step / tile / point / smoothing /
// regularisation objects keep their pinned kernel counts.
//
// Lane = trace: every global load and store runs along the fast axis.  A block of 256 threads owns FIR_LANES = 64 traces
// by FIR_TT = 32 output times; each of its four waves keeps FIR_TO = 8 consecutive output times per lane in registers.
// The taps b_0 .. b_R sit in LDS (at most 4097 doubles).  The input rows t0 - R .. t0 + FIR_TT + R - 1 that the tile
// needs do not fit LDS at the R of a real band-pass, so they pass through it in chunks of FIR_CH = 32 rows, in ascending
// time: per chunk
//   stage   x = [wpre .] (in - sub) of the chunk's rows as fp64; rows outside [0, nt) and traces >= ntr are not read,
//           their slots hold zeros;
//   sum     per 8 rows: the 15 taps b_|k| that 8 rows and 8 outputs can pair (zero where |k| > R) go to registers, then
//           every row's x is read once from LDS and added into the 8 accumulators: 64 fp64 FMAs for 23 LDS reads.
// For every output the terms are added over ascending k, in fp64; the result is rounded to T once, when it is stored.
// The squares of the unrounded outputs (of the stored, rounded ones where the caller asks: the plain residual, whose J is
// then fwi_misfit_l2's) are summed per thread over ascending time, over the block by a fixed tree into partial[block];
// fir_sum adds the partials in a fixed order.  No atomics.
#include <hip/hip_runtime.h>

#include "fwi_data.h"

namespace fwi {

namespace {

constexpr int FIR_BLOCK = 256, FIR_CH = 32;
static_assert(FIR_BLOCK == 64 * (FIR_TT / FIR_TO) && FIR_LANES == 64, "one wave per FIR_TO output times");
static_assert(FIR_CH % FIR_TO == 0 && FIR_CH * FIR_LANES >= FIR_BLOCK, "whole groups of rows; room for the block's sum");

struct FirArgs {
    int nt, ntr, R, xtiles;
    int sq_stored;  // sum the squares of the outputs as stored (rounded to T), not of the fp64 values
};

template <typename T>
__global__ __launch_bounds__(FIR_BLOCK) void fir_time(T *out, const T *in, const T *sub, const T *wpre, const T *wpost,
                                                      const double *taps, FirArgs a, double *partial) {
    extern __shared__ double smem[];
    double *sX = smem;                       // [FIR_CH][FIR_LANES]
    double *sB = smem + FIR_CH * FIR_LANES;  // [R + 1]
    const int tid = threadIdx.x, lane = tid & 63, grp = tid >> 6;
    const int x0 = (int)(blockIdx.x % a.xtiles) * FIR_LANES, t0 = (int)(blockIdx.x / a.xtiles) * FIR_TT;
    const int gx = x0 + lane, tn0 = t0 + grp * FIR_TO;  // this thread's trace and its first output time
    const int R = a.R;
    for (int k = tid; k <= R; k += FIR_BLOCK) sB[k] = taps ? taps[k] : 1.0;
    double acc[FIR_TO];
#pragma unroll
    for (int j = 0; j < FIR_TO; ++j) acc[j] = 0.0;

    const int lo = t0 - R > 0 ? t0 - R : 0, hi = t0 + FIR_TT + R < a.nt ? t0 + FIR_TT + R : a.nt;
    for (int m0 = lo; m0 < hi; m0 += FIR_CH) {
        __syncthreads();  // the chunk before is used up
        for (int i = tid; i < FIR_CH * FIR_LANES; i += FIR_BLOCK) {
            const int gm = m0 + (i >> 6), g = x0 + (i & 63);
            double v = 0.0;
            if (gm < hi && g < a.ntr) {
                const int64_t at = (int64_t)gm * a.ntr + g;
                v = (double)in[at];
                if (sub) v -= (double)sub[at];
                if (wpre) v *= (double)wpre[at];
            }
            sX[i] = v;
        }
        __syncthreads();
#pragma unroll 1
        for (int mb = 0; mb < FIR_CH; mb += FIR_TO) {
            const int d0 = m0 + mb - tn0;  // k = row - output of (row mb, output 0): the group pairs k in d0 - 7 .. d0 + 7
            if (m0 + mb >= hi || d0 + (FIR_TO - 1) < -R || d0 - (FIR_TO - 1) > R) continue;  // (the same for a whole wave)
            double w[2 * FIR_TO - 1];
#pragma unroll
            for (int q = 0; q < 2 * FIR_TO - 1; ++q) {
                const int k = d0 + q - (FIR_TO - 1), kk = k < 0 ? -k : k;
                w[q] = kk <= R ? sB[kk] : 0.0;
            }
#pragma unroll
            for (int i = 0; i < FIR_TO; ++i) {
                const double xv = sX[(mb + i) * FIR_LANES + lane];
#pragma unroll
                for (int j = 0; j < FIR_TO; ++j) acc[j] = fma(w[i - j + FIR_TO - 1], xv, acc[j]);
            }
        }
    }

    double sq = 0.0;
    if (gx < a.ntr) {
#pragma unroll
        for (int j = 0; j < FIR_TO; ++j) {
            if (tn0 + j < a.nt) {
                const int64_t at = (int64_t)(tn0 + j) * a.ntr + gx;
                double v = acc[j];
                if (wpost) v *= (double)wpost[at];
                const T o = (T)v;
                out[at] = o;
                if (a.sq_stored) v = (double)o;
                sq += v * v;
            }
        }
    }
    if (partial) {
        __syncthreads();  // the last chunk is used up: its LDS takes the block's sum
        sX[tid] = sq;
        __syncthreads();
        for (int s = FIR_BLOCK / 2; s > 0; s >>= 1) {
            if (tid < s) sX[tid] += sX[tid + s];
            __syncthreads();
        }
        if (tid == 0) partial[blockIdx.x] = sX[0];
    }
}

// partial[n] = sum of partial[0 .. n): strided per thread, then a fixed tree
__global__ __launch_bounds__(FIR_BLOCK) void fir_sum(double *partial, int64_t n) {
    __shared__ double sRed[FIR_BLOCK];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int64_t i = tid; i < n; i += FIR_BLOCK) acc += partial[i];
    sRed[tid] = acc;
    __syncthreads();
    for (int s = FIR_BLOCK / 2; s > 0; s >>= 1) {
        if (tid < s) sRed[tid] += sRed[tid + s];
        __syncthreads();
    }
    if (tid == 0) partial[n] = sRed[0];
}

}  // namespace

int64_t fir_blocks(int nt, int ntr) {
    return (int64_t)((ntr + FIR_LANES - 1) / FIR_LANES) * ((nt + FIR_TT - 1) / FIR_TT);
}

template <typename T>
hipError_t launch_fir_time(T *out, const T *in, const T *sub, const T *wpre, const T *wpost, const double *taps, int R,
                           int nt, int ntr, double *partial, bool sq_stored, hipStream_t s) {
    const int64_t blocks = fir_blocks(nt, ntr);
    if (!out || !in || nt < 1 || ntr < 1 || R < 0 || R > FIR_RMAX || blocks > 0x7fffffff || out == in || out == sub ||
        out == wpre || out == wpost)
        return hipErrorInvalidValue;
    FirArgs a;
    a.nt = nt, a.ntr = ntr, a.xtiles = (ntr + FIR_LANES - 1) / FIR_LANES;
    a.R = !taps ? 0 : R < nt - 1 ? R : nt - 1;  // the taps beyond nt - 1 meet no sample
    a.sq_stored = sq_stored ? 1 : 0;
    const size_t lds = (size_t)(FIR_CH * FIR_LANES + a.R + 1) * sizeof(double);
    hipLaunchKernelGGL(fir_time<T>, dim3((unsigned)blocks), dim3(FIR_BLOCK), lds, s, out, in, sub, wpre, wpost, taps, a,
                       partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !partial) return e;
    hipLaunchKernelGGL(fir_sum, dim3(1), dim3(FIR_BLOCK), 0, s, partial, blocks);
    return hipGetLastError();
}

template hipError_t launch_fir_time<float>(float *, const float *, const float *, const float *, const float *,
                                           const double *, int, int, int, double *, bool, hipStream_t);
template hipError_t launch_fir_time<double>(double *, const double *, const double *, const double *, const double *,
                                            const double *, int, int, int, double *, bool, hipStream_t);

}  // namespace fwi
