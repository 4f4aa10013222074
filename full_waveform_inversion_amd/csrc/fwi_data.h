// Band-limited, weighted least-squares data misfit (fwi_misfit_weighted, fwi_residual_weight): a symmetric FIR filter
// along time applied to (nt, ntr) trace gathers, time the slow axis, the trace index the fast one.  Internal launch
// interface between fwi_api_misfit.hip and fwi_data.hip.
//
//   (B x)[n, j] = sum_{k = -R .. R} b_|k| x[n + k, j],   terms with n + k outside [0, nt) omitted (zero extension):
//   B is a symmetric matrix, B^T = B.
//
// No reference counterpart.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fwi {

constexpr int FIR_RMAX = 4096;  // largest half-width the entry points accept

// out :=[wpost .] B([wpre .] (in - sub)) over (nt, ntr); sub, wpre and wpost may each be nullptr (no subtraction, weight
// 1).  taps: R + 1 doubles b_0 .. b_R on the device, nullptr: B = I (R is then ignored).  R may exceed nt - 1: the taps
// beyond are never read.  Everything between the loads and the one rounding to T is fp64, summed over ascending k.
// partial != nullptr: partial[gather_blocks] := sum of the squares of the UNROUNDED output values -- sq_stored: of the
// values as stored, rounded to T, which is what fwi_misfit_l2 sums -- added over the blocks' partial sums
// partial[0 .. gather_blocks) in a fixed order (fwi_gather_tile.h has the tile and the sums): equal inputs give equal
// bits.  out must not alias in, sub or the weights (tiles read their neighbours' rows).  Rows outside [0, nt) and
// traces >= ntr are never read.
template <typename T>
hipError_t launch_fir_time(T *out, const T *in, const T *sub, const T *wpre, const T *wpost, const double *taps, int R,
                           int nt, int ntr, double *partial, bool sq_stored, hipStream_t s);

}  // namespace fwi
