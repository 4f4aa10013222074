// First-order Tikhonov and smoothed isotropic total-variation regularisation of a compact model-sized vector
// (fwi_vec_regularizer).  Internal launch interface between fwi_api_vec.hip and fwi_reg.hip.
//
//   d = x - x0 (or x),  (D_a d)_i = d_{i+e_a} - d_i for i_a < n_a - 1, 0 on the last cell of the axis (nx, not cx),
//   s_i = sum_a w_a (D_a d)_i^2,
//   Tikhonov  R = 1/2 sum_i s_i,                      k_i = 1,
//   TV        R = sum_i (sqrt(s_i + eps^2) - eps),    k_i = 1 / sqrt(s_i + eps^2),
//   L(d; v)_j = sum_a w_a [k_{j-e_a} (D_a v)_{j-e_a} - k_j (D_a v)_j].
//
// No reference counterpart.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fwi_kernels.h"

namespace fwi {

constexpr int REG_TIKHONOV = 0, REG_TV = 1;
// A block of 256 threads owns REG_TY rows of 16 lanes of 16 bytes (64 fp32 / 32 fp64 columns) and marches over REG_ZC
// planes.  A 2-D grid (nz, nx) is the 3-D grid (1, nz, nx).
constexpr int REG_TY = 16, REG_XL = 16, REG_ZC = 16;

// number of blocks of one launch = number of partial sums; the buffer handed over holds one double more (the total)
template <typename T>
int64_t reg_blocks(const GridDesc &g);

// out := alpha L(d; v) + beta out (out == nullptr: nothing written; beta == 0: out is not read), and
// partial[reg_blocks] := R(d), summed over the blocks' partial sums partial[0 .. reg_blocks) in a fixed order: equal
// inputs give equal bits.  x0 == nullptr: d = x.  v == nullptr: v = d.  w: the weights of z, y, x (2-D: w[1] unused).
// out must not alias x, x0 or v.  Pad columns of out are written as zeros; those of the inputs are never used.
template <typename T>
hipError_t launch_regularizer(const GridDesc &g, int kind, T *out, const T *x, const T *x0, const T *v, double alpha,
                              double beta, const double w[3], double eps, double *partial, hipStream_t s);

}  // namespace fwi
