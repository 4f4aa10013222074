// Extended Born modelling on the Fourier store (include/fwi.h, fwi_fourier_born_extended[_vec]): the scattering spectrum
// P_k of a gather (E_l)_l, the transpose of the extended images of fwi_feximage.h, one lag per launch.  Internal launch
// interface between fwi_api.hip and fwi_fbornx.hip.
//
//   offset  P_k(y) (+)= E(y - h e) Q_k(y - 2 h e)   where y - h e and y - 2 h e are both cells of the grid, else nothing
//   lag     P_k(y) (+)= E(y) Q_k(y) exp(-i phi_k),  phi_k = 2 pi f_k tau
//
// `p`, `q`: 2 F compact volumes each in the layout of fwi_fourier.h (Re at 2 k npts, Im at (2 k + 1) npts), in the
// context dtype; `img`: one compact volume (pad columns zero).  `beta` = 0: p is written and never read (the first lag;
// cells without a contribution and the pad columns get zeros), else the lag is added to what p holds.  `cs`: 2 F doubles
// on the device, cos phi_k at k and sin phi_k at F + k, read at the same address in every lane.  `axis`: 0 = z, 1 = y,
// 2 = x of the GridDesc (not the caller's grid order); `h`: any integer of 32 bits, in cells.  Per cell the products are
// formed in fp64 and rounded once to the context dtype:
//   offset  Re P = T(fma(E, Re Q, Re P)), Im P = T(fma(E, Im Q, Im P))
//   lag     Re P = T(fma(E, fma(Im Q, sin, Re Q * cos), Re P)), Im P = T(fma(E, fma(-Re Q, sin, Im Q * cos), Im P))
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fwi_kernels.h"

namespace fwi {

// one read of img and of the 2 F volumes of q where the shifted cells exist, one write (beta: read and write) of p
template <typename T>
hipError_t launch_fbornx_offset(const GridDesc &g, T *p, const T *q, const T *img, int F, int axis, int64_t h, int beta,
                                hipStream_t s);

// one read of img and of the 2 F volumes of q, one write (beta: read and write) of the 2 F volumes of p
template <typename T>
hipError_t launch_fbornx_lag(T *p, const T *q, const T *img, const double *cs, int64_t npts, int F, int beta,
                             hipStream_t s);

}  // namespace fwi
