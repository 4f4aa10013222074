// Extended images on the Fourier store (include/fwi.h, fwi_fourier_offset_image[_vec] and fwi_fourier_lag_image[_vec]):
// subsurface-offset and time-lag common-image gathers from the coefficients Q_k of the forward term and M_k of the
// adjoint field, one lag per launch.  Internal launch interface between fwi_api_fourier.hip and fwi_feximage.hip.
//
//   offset  dst(x) = sum_k a_k (Re Q_k(x - h e) Re M_k(x + h e) + Im Q_k(x - h e) Im M_k(x + h e))
//           where x - h e and x + h e are both cells of the grid, 0 elsewhere and in the pad columns
//   lag     dst(x) = sum_k (C_k Re P_k(x) + D_k Im P_k(x)),  P_k = Q_k conj M_k
//
// `q`, `m`: 2 F compact volumes each in the layout of fwi_fourier.h (Re at 2 k npts, Im at (2 k + 1) npts), in the
// context dtype; `dst`: one compact volume, written and never read.  `a`: F doubles on the device, the caller's weight
// times w_k; `cd`: 2 F doubles, C_k = a_k cos phi_k at k and D_k = a_k sin phi_k at F + k, phi_k = 2 pi f_k tau; both are
// read at the same address in every lane.  `axis`: 0 = z, 1 = y, 2 = x of the GridDesc (not the caller's grid order);
// `h`: any integer, in cells.  The offset sum on the sampled histories is sum_j mu^{jS+1}(x + h e) q~^{jS}(x - h e) for
// any set of frequencies.  The lag sum is the imaging sum with q~ delayed circularly by m samples only where every f_k is
// a bin of the sampled axis and tau = m S dt; off the bins, or at other tau, it is this formula and no such sum.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fwi_kernels.h"

namespace fwi {

// one read of each of the 4 F volumes where both shifted cells exist, one write of dst
template <typename T>
hipError_t launch_feximage_offset(const GridDesc &g, T *dst, const T *q, const T *m, const double *a, int F, int axis,
                                  int64_t h, hipStream_t s);

// one read of each of the 4 F volumes, one write of dst
template <typename T>
hipError_t launch_feximage_lag(T *dst, const T *q, const T *m, const double *cd, int64_t npts, int F, hipStream_t s);

}  // namespace fwi
