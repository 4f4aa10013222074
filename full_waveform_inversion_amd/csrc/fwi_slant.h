// The slant stack over vector slots (include/fwi.h, fwi_vec_shift_sum): one compact volume from up to SLANT_MAX others,
// each shifted along z by a real number of cells.  Internal launch interface between fwi_api_vec.hip and fwi_slant.hip.
//
//   dst := beta dst + sum_{i < nsrc} (c0_i src_i(z + n_i, .) + c1_i src_i(z + n_i + 1, .))
//
// For the shift s_i = n_i + f_i (n_i = floor(s_i), 0 <= f_i < 1) and the weight w_i the caller forms c0_i = w_i (1 - f_i)
// and c1_i = w_i f_i in fp64.  A tap whose plane lies outside 0 .. nz - 1 contributes nothing and is not read; the second
// tap is neither read nor counted where c1_i == 0.  `src`: compact volumes of the context dtype (separate allocations,
// the same one may appear twice), none of them `dst`; `dst` is not read where beta == 0, and its pad columns are
// written as zeros.  |n_i| <= nz + 1: a source further out contributes nothing and is dropped by the caller, so that
// n_i times the plane pitch is an offset inside 64 bits (the launcher refuses any other).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fwi_kernels.h"

namespace fwi {

constexpr int SLANT_MAX = 64;  // FWI_SHIFT_SUM_MAX of include/fwi.h

// passed by value in the kernel arguments (2 KiB): every entry is read at the same address in all lanes
struct SlantTable {
    const void *src[SLANT_MAX];
    int64_t n[SLANT_MAX];
    double c0[SLANT_MAX], c1[SLANT_MAX];
};

// one read of each source plane a tap of which lies in the grid, one read of dst where beta != 0, one write of dst;
// nsrc = 0: dst := beta dst alone
template <typename T>
hipError_t launch_slant_sum(const GridDesc &g, T *dst, const SlantTable &t, int nsrc, double beta, hipStream_t s);

}  // namespace fwi
