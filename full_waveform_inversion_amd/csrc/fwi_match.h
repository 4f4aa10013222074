// Matching-filter (source-independent) data misfit (fwi_misfit_matched): the normal equations of a short two-sided
// filter along time between two (nt, ntr) gathers, and the filter's convolution / correlation with a gather.  Time is
// the slow axis, the trace index the fast one.  Internal launch interface between fwi_api_misfit.hip and fwi_match.hip.
//
//   f = (f_-L .. f_L), K = 2 L + 1 coefficients, stored f[k + L]
//   (C_f x)[n, j]   = sum_{k = -L .. L} f_k x[n - k, j]      terms with n - k outside [0, nt) omitted
//   (C_f^T y)[m, j] = sum_{k = -L .. L} f_k y[m + k, j]      terms with m + k outside [0, nt) omitted
//   G[k, l] = sum_{n, j} M^2[n, j] s[n - k, j] s[n - l, j],    b[k] = sum_{n, j} M^2[n, j] s[n - k, j] d[n, j]
//
// G is not Toeplitz (the weights and the truncation at both ends of the trace), and is formed as defined.
//
// No reference counterpart.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fwi {

constexpr int MATCH_LMAX = 64;  // largest half-length the entry points accept (FWI_MATCH_LMAX)

// doubles of the partials buffer launch_match_normal needs for this gather and L (at most 256 slices of
// 64 P + 8 nT doubles, nT = ceil(K / 8), P = nT (nT + 1) / 2: 20 MB at L = 64)
int64_t match_normal_partials(int nt, int ntr, int L);

// normal[0 .. K K) := G, row-major, full and exactly symmetric (the upper triangle is computed, the lower copied);
// normal[K K .. K K + K) := b.  s, d: (nt, ntr); w: the weights M (nullptr: 1); M^2 is formed in fp64.  Everything is
// fp64; every entry is summed in an order that depends on (nt, ntr, L) only -- per wave over its samples in ascending
// time, over the wave's lanes by a fixed tree, over the slices of `partial` in ascending order: no atomics, equal inputs
// give equal bits.  Rows outside [0, nt) and traces >= ntr are never read.  L may exceed nt - 1.
template <typename T>
hipError_t launch_match_normal(double *normal, double *partial, const T *s, const T *d, const T *w, int L, int nt,
                               int ntr, hipStream_t st);

// out := [wpost .] (C ([wpre .] in) [- sub]) over (nt, ntr), C = C_f, or C_f^T with `corr`; f: K doubles on the device.
// Per output the terms are added over ascending k in fp64; the result is rounded to T once, at the store.
// partial != nullptr: partial[gather_blocks] := the sum of the squares of the unrounded outputs, added in a fixed
// order (fwi_gather_tile.h has the tile and the sums).  out must not alias an input.
template <typename T>
hipError_t launch_match_apply(T *out, const T *in, const T *sub, const T *wpre, const T *wpost, const double *f, int L,
                              bool corr, int nt, int ntr, double *partial, hipStream_t st);

}  // namespace fwi
