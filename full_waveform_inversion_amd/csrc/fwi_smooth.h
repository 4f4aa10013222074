// Separable Gaussian smoothing of a compact model-sized vector (fwi_vec_smooth).  Internal launch interface between
// fwi_api_vec.hip and fwi_smooth.hip.
//
//   (S_sigma x)_i = sum_{k = -R .. R} w_|k| x_rho(i + k),   R = int(3 sigma + 0.5),
//   w_k = exp(-k^2 / 2 sigma^2) / sum_j exp(-j^2 / 2 sigma^2),
//   rho the half-sample mirror of the axis (rho(j) = -1 - j below 0, 2 n - 1 - j from n on; R <= n: one reflection).
//
// This is scipy.ndimage.gaussian_filter(mode="reflect", truncate=3.0) axis by axis.  No reference counterpart.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fwi_kernels.h"

namespace fwi {

constexpr int SMOOTH_RMAX = 32;  // widest radius of one pass (sigma <= 10.8); apply the operator twice beyond it

// R of a width (the caller has checked that sigma is finite and >= 0)
inline int smooth_radius(double sigma) { return (int)(3.0 * sigma + 0.5); }

// the R + 1 weights w_0 .. w_R in fp64 (w[k] = w[-k]; their sum over -R .. R is 1)
void smooth_weights(double sigma, int R, double *w);

// dst = S src along one axis (0 = z, 1 = y, 2 = x; a 2-D grid has no axis 1) of the compact layout: the mirror is taken
// against the axis' logical length (nx, not cx), the cx - nx pad columns of dst are written as zeros.  `w`: R + 1 weights
// on the HOST, already rounded to T (they travel as kernel arguments).  dst must not alias src; every element of dst
// is written.  1 <= R <= min(SMOOTH_RMAX, length of the axis), else hipErrorInvalidValue.  The summation order is
// fixed (ascending source index), so the result does not depend on the launch.
template <typename T>
hipError_t launch_smooth_axis(const GridDesc &g, T *dst, const T *src, int axis, int R, const T *w, hipStream_t s);

}  // namespace fwi
