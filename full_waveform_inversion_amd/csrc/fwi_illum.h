// Source-side illumination (the diagonal of the pseudo-Hessian, Shin et al. 2001) and the two vector operations that
// turn it into a preconditioner.  Internal launch interface between the host units (fwi_api.hip, fwi_api_fourier.hip, fwi_api_vec.hip) and fwi_illum.hip.
//
//   acc(x) += sum over nslots compact store slots of q(x)^2      (slot k at store + k * npts * qes bytes)
//   H_m(x)  = (S / dt^4) acc(x)                                  (finalize, S = image stride)
//   H_c(x)  = H_m(x) (2 / c(x)^3)^2
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fwi_kernels.h"

namespace fwi {

// acc[i] += sum_k q_k[i]^2 over `nslots` slots of a native (q_bf16 = 0) or bf16 (fp32 contexts) store.  One launch
// reads every slot once and read-modify-writes acc once.
template <typename T>
hipError_t launch_illum_accumulate(T *acc, const void *store, int64_t npts, int nslots, int q_bf16, hipStream_t s);

// bf16 store: the stored term is b = bf16(C L u); the source's share c = sum_j cq_j w_j^n (entries j at the node)
// is added exactly, so acc(x_s) += sum_n (2 b c + c^2) over the imaging steps n % stride == 0, slot n / stride.
hipError_t launch_illum_source_bf16(float *acc, const void *store, int64_t npts, const float *wav, const int64_t *cidx,
                                    const float *cq, int nt, int nsrc, int stride, hipStream_t s);

// out = scale * acc (slowness^2) or scale * acc * 4 / c^6 (velocity); pad columns 0
template <typename T>
hipError_t launch_illum_finalize(const GridDesc &g, const T *acc, const T *c, T *out, double scale, int wrt_velocity,
                                 hipStream_t s);

// y := x * y and y := a / (y + b), elementwise over the compact layout (pad columns stay 0)
template <typename T>
hipError_t launch_vec_mul(const GridDesc &g, T *y, const T *x, hipStream_t s);
template <typename T>
hipError_t launch_vec_recip(const GridDesc &g, T *y, double a, double b, hipStream_t s);

}  // namespace fwi
