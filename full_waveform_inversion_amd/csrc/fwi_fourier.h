// Fourier-compressed forward-term store (include/fwi.h, fwi_set_fourier_store): the two streaming transforms along the
// sampled time axis.  Internal launch interface between fwi_api.hip and fwi_fourier.hip.
//
//   analysis   Re Q_k(x) += sum_b q^{(j0+b) S}(x) cos theta_{k, j0+b}
//              Im Q_k(x) -= sum_b q^{(j0+b) S}(x) sin theta_{k, j0+b}              b = 0 .. nb - 1, k = 0 .. F - 1
//   synthesis  q~^{(j0+b) S}(x) = sum_k w_k (Re Q_k(x) cos theta_{k, j0+b} - Im Q_k(x) sin theta_{k, j0+b})
//
// `acc`: 2 F compact volumes, Re Q_k at acc + 2 k npts, Im Q_k at acc + (2 k + 1) npts, in the context dtype.  `ring`:
// `ring_slots` compact volumes, sample j in slot j % ring_slots; `slot0` = j0 % ring_slots.  `tw`: the fp64 table of
// the sweep on the device, frequency-major: F blocks of `tw_rows` (cos, sin) pairs, row j of block k =
// (cos theta_kj, sin theta_kj) for the analysis and the same times the weight w_k for the synthesis.  A batch always
// reads FOURIER_BMAX consecutive rows (128 contiguous bytes per frequency), so tw_rows >= N + FOURIER_BMAX - 1 and the
// rows from N on hold zeros.  The host forms the table (fwi_api.hip, fourier_table); the kernels only read it, at the
// same address in every lane.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fwi {

constexpr int FOURIER_BMAX = 8;  // samples per batch (FWI_FOURIER_BMAX): one register set per sample and cell

// `nb` <= FOURIER_BMAX samples j0 .. j0 + nb - 1: one read of their slots, one read-modify-write of every accumulator
template <typename T>
hipError_t launch_fourier_analyse(T *acc, const T *ring, int64_t npts, int ring_slots, int slot0, int j0, int nb,
                                  const double *tw, int tw_rows, int F, hipStream_t s);

// one read of every accumulator, one write of the slots of the samples j0 .. j0 + nb - 1
template <typename T>
hipError_t launch_fourier_synthesise(T *ring, const T *acc, int64_t npts, int ring_slots, int slot0, int j0, int nb,
                                     const double *tw, int tw_rows, int F, hipStream_t s);

}  // namespace fwi
