// Spectral imaging on the Fourier-compressed forward-term store (include/fwi.h, fwi_adjoint_spectral and
// fwi_fourier_image / _gradient / _illumination): the gradient is formed per frequency from the coefficients Q_k of the
// forward term and M_k of the adjoint field.  Internal launch interface between the host units (fwi_api.hip, fwi_api_fourier.hip) and fwi_fimage.hip.
//
//   pack        slot(x) = mu(x) for the grid's cells, 0 in the pad columns: a padded field into one compact ring slot
//   image       dst(x) = beta dst(x) + sum_k a_k (Re Q_k(x) Re M_k(x) + Im Q_k(x) Im M_k(x))
//   illuminate  dst(x) = beta dst(x) + sum_k a_k (Re Q_k(x)^2 + Im Q_k(x)^2)
//
// `q`, `m`: 2 F compact volumes each in the layout of fwi_fourier.h (Re at 2 k npts, Im at (2 k + 1) npts), in the
// context dtype; `dst`: one compact volume.  `a`: F doubles on the device, the caller's weight times w_k, read at the
// same address in every lane.  `beta` is 0 (dst is written, never read) or 1.  M_k itself comes from
// launch_fourier_analyse on the slots the pack kernel fills.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fwi_kernels.h"

namespace fwi {

// one padded read of the grid's cells, one write of the slot
template <typename T>
hipError_t launch_fimage_pack(const GridDesc &g, const T *u, T *slot, hipStream_t s);

// one read of each of the 4 F volumes; dst: one write (beta = 0) or one read-modify-write (beta = 1)
template <typename T>
hipError_t launch_fimage_image(T *dst, const T *q, const T *m, const double *a, int64_t npts, int F, int beta,
                               hipStream_t s);

// one read of each of the 2 F volumes of q; dst as above
template <typename T>
hipError_t launch_fimage_illuminate(T *dst, const T *q, const double *a, int64_t npts, int F, int beta, hipStream_t s);

}  // namespace fwi
