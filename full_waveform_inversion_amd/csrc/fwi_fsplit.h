// The tomographic / migration split of the spectral image on the Fourier store (include/fwi.h,
// fwi_fourier_split_image[_vec]).  Internal launch interface between fwi_api_fourier.hip and fwi_fsplit.hip.
//
// With the one-sided taps t_1 .. t_R and an axis a of the grid, (H u)(i) = sum_{r = 1 .. R} t_r (u(i - r) - u(i + r))
// along that axis, cells outside [0, n_a) of the GRID contributing nothing (zero extension; the pad columns of a compact
// row are no cells), taps that are exactly zero skipped, H acting on Re and Im separately:
//
//   dst(x) = sum_k a_k [ alpha (Re Q_k Re M_k + Im Q_k Im M_k) + beta (Re HQ_k Re HM_k + Im HQ_k Im HM_k) ]
//
// and 0 in the pad columns.  (alpha, beta) = (1/2, 1/2): the pairs of equal direction along the axis (low wavenumber,
// tomographic); (1/2, -1/2): the pairs of opposite direction (high wavenumber, migration); (0, 1): the image of the
// filtered coefficients alone.
//
// `q`, `m`: 2 F compact volumes each in the layout of fwi_fourier.h (Re at 2 k npts, Im at (2 k + 1) npts), in the
// context dtype; `dst`: one compact volume, written and never read.  `a`: F doubles on the device, the caller's weight
// times w_k; `taps`: `ntaps` doubles on the device, t_r at r - 1; both are read at the same address in every lane.
// `axis`: 0 = z, 1 = y, 2 = x of the GridDesc (not the caller's grid order).  0 <= ntaps <= FSPLIT_RMAX; the caller drops
// the taps at r >= n_a (they touch nothing), so ntaps < n_a.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fwi_kernels.h"

namespace fwi {

constexpr int FSPLIT_RMAX = 64;   // FWI_SPLIT_RMAX of include/fwi.h
constexpr int FSPLIT_CHUNK = 64;  // cells along z or y that one workgroup forms, from CHUNK + 2 ntaps staged rows

// one read of each of the 4 F volumes plus the halo rows of the tiling (fwi_fsplit.hip), one write of dst
template <typename T>
hipError_t launch_fsplit(const GridDesc &g, T *dst, const T *q, const T *m, const double *a, int F, int axis,
                         const double *taps, int ntaps, double alpha, double beta, hipStream_t s);

}  // namespace fwi
