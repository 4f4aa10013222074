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

// ---- imaging Born operator on decimated / bf16 stores (fwi_born_bf16.hip; include/fwi.h, fwi_born_imaging) ----------
// launch_born_weight with the quadrature weight of a strided store folded in: w = stride * dC / C (formed in double, rounded
// once), so that no step of the sweep needs an extra multiply.
template <typename T>
hipError_t launch_born_weight_strided(const GridDesc &g, const T *dm, const T *c, T *w, int wrt_velocity, int stride,
                                      hipStream_t s);

// launch_born_scatter (standard form) with q read from a bf16 store: four bf16 values = 8 bytes per lane against the
// 16-byte field vectors.  fp32 only, as the bf16 store is.
hipError_t launch_born_scatter_bf16(const GridDesc &g, float *u, const void *q_bf16, const float *w, const float *dz,
                                    const float *dy, const float *dx, int damp, hipStream_t s);

// bf16 store: the source's own share C src^n of the forward term is not in the store (it holds bf16(C L u^n)); the Born
// sweep injects w(x_s) C src^n(x_s) at the source nodes through the step launch's fused injection, whose amplitudes are
// out[n, s] = w[cidx[s]] * wav[n, s]  (the injection multiplies by A C / h^D and sums the entries of one node first).
hipError_t launch_born_source_share(const float *w, const int64_t *cidx, const float *wav, float *out, int nt, int nsrc,
                                    hipStream_t s);

}  // namespace fwi
