// Symmetric FIR filtering along time of (nt, ntr) trace gathers, with optional per-sample weights before and after the
// filter and a reproducible sum of squares (fwi_data.h).  Its own object: the step / tile / point / smoothing /
// regularisation objects keep their pinned kernel counts.
//
// The tile, the march of the input rows through LDS in chunks of FIR_CH = 32 rows and the fixed-order sums are the
// shared ones of fwi_gather_tile.h; the taps b_0 .. b_R sit in LDS behind the chunk (at most 4097 doubles).  Staging
// forms x = [wpre .] (in - sub) as fp64.  The result is rounded to T once, when it is stored.  The squares of the
// unrounded outputs (of the stored, rounded ones where the caller asks: the plain residual, whose J is then
// fwi_misfit_l2's) are what the thread sums.
#include <hip/hip_runtime.h>

#include "fwi_data.h"
#include "fwi_gather_tile.h"
#include "fwi_kernels.h"

namespace fwi {

namespace {

constexpr int FIR_CH = 32;

struct FirArgs {
    int nt, ntr, R, xtiles;
    int sq_stored;  // sum the squares of the outputs as stored (rounded to T), not of the fp64 values
};

template <typename T>
__global__ __launch_bounds__(GT_BLOCK) void fir_time(T *out, const T *in, const T *sub, const T *wpre, const T *wpost,
                                                     const double *taps, FirArgs a, double *partial) {
    extern __shared__ double smem[];
    double *sX = smem;                      // [FIR_CH][GT_LANES]
    double *sB = smem + FIR_CH * GT_LANES;  // [R + 1]
    const GatherTile c = gather_tile(a.xtiles);
    for (int k = threadIdx.x; k <= a.R; k += GT_BLOCK) sB[k] = taps ? taps[k] : 1.0;
    double acc[1][GT_TO];
    gather_march<1, FIR_CH>(acc, sX, c, a.nt, a.ntr, [&](int, int64_t at) {
        double v = (double)in[at];
        if (sub) v -= (double)sub[at];
        if (wpre) v *= (double)wpre[at];
        return v;
    }, SymmetricTaps{sB, a.R});

    double sq = 0.0;
    if (c.gx < a.ntr) {
#pragma unroll
        for (int j = 0; j < GT_TO; ++j) {
            if (c.tn0 + j < a.nt) {
                const int64_t at = (int64_t)(c.tn0 + j) * a.ntr + c.gx;
                double v = acc[0][j];
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
        block_tree_sum_to_partial(sq, sX, partial);
    }
}

}  // namespace

template <typename T>
hipError_t launch_fir_time(T *out, const T *in, const T *sub, const T *wpre, const T *wpost, const double *taps, int R,
                           int nt, int ntr, double *partial, bool sq_stored, hipStream_t s) {
    const int64_t blocks = gather_blocks(nt, ntr);
    if (!out || !in || nt < 1 || ntr < 1 || R < 0 || R > FIR_RMAX || blocks > 0x7fffffff || out == in || out == sub ||
        out == wpre || out == wpost)
        return hipErrorInvalidValue;
    FirArgs a;
    a.nt = nt, a.ntr = ntr, a.xtiles = gather_xtiles(ntr);
    a.R = !taps ? 0 : R < nt - 1 ? R : nt - 1;  // the taps beyond nt - 1 meet no sample
    a.sq_stored = sq_stored ? 1 : 0;
    const size_t lds = (size_t)(FIR_CH * GT_LANES + a.R + 1) * sizeof(double);
    hipLaunchKernelGGL(fir_time<T>, dim3((unsigned)blocks), dim3(GT_BLOCK), lds, s, out, in, sub, wpre, wpost, taps, a,
                       partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !partial) return e;
    return launch_sum_partials(partial, blocks, s);
}

template hipError_t launch_fir_time<float>(float *, const float *, const float *, const float *, const float *,
                                           const double *, int, int, int, double *, bool, hipStream_t);
template hipError_t launch_fir_time<double>(double *, const double *, const double *, const double *, const double *,
                                            const double *, int, int, int, double *, bool, hipStream_t);

}  // namespace fwi
