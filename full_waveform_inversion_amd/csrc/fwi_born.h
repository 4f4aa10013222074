// Born (linearised) modelling: the two kernels that turn a forward sweep's store into J dm (fwi_born.hip).  Internal
// launch interface between fwi_api.hip and fwi_born.hip.
//
// The Born field obeys the recursion of the wavefield with the distributed source w q^n in the place of the point
// source, w = dC / C and q^n the stored forward term (include/fwi.h, fwi_born).  A Born sweep therefore runs the
// ordinary one-step launches on a zeroed field and, after step n,
//     du^{n+1} += A w q^n          (increment form: dv^{n+1} += the same)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fwi_kernels.h"

namespace fwi {

// w = 2 dm / c (wrt_velocity) or -c^2 dm (dm a perturbation of 1 / c^2), compact layout, pad columns 0.  `w` may be
// the array `dm` itself.
template <typename T>
hipError_t launch_born_weight(const GridDesc &g, const T *dm, const T *c, T *w, int wrt_velocity, hipStream_t s);

// u (padded) += A w q at the grid's interior points, q and w compact; v (padded; nullptr = standard form) takes the same
// increment.  A = 1 / (1 + dz[z] + dy[y] + dx[x]) with `damp`, 1 without (no border, or the convolutional PML).  Halo,
// pad columns, look-ahead planes and tail of the padded fields are never written.
template <typename T>
hipError_t launch_born_scatter(const GridDesc &g, T *u, T *v, const T *q, const T *w, const T *dz, const T *dy,
                               const T *dx, int damp, hipStream_t s);

}  // namespace fwi
