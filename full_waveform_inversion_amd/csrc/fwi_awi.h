// Adaptive (per-trace matching-filter) misfit (fwi_misfit_adaptive; Warner & Guasch 2016) of (nt, ntr) trace gathers, time
// the slow axis, the trace index the fast one: per trace the Wiener filter that turns the data into the synthetics, its
// second moment about zero lag and the adjoint source.  Internal launch interface between fwi_api_misfit.hip and
// fwi_awi.hip.
//
//   sh = M . s,  dh = M . d                        (s, d: the gathers after the filter B, where there is one)
//   L >= 1,  K = 2 L + 1,  every trace zero-extended outside [0, nt)
//   a_j(m) = sum_n dh[n, j] dh[n + m, j],  m = 0 .. 2 L          c_j(k) = sum_n sh[n + k, j] dh[n, j],  k = -L .. L
//   G_j[k, l] = a_j(|k - l|) + lam a_j(0) [k == l]               w_j = G_j^-1 c_j
//   N_j = sum_k w_k^2,  W_j = sum_k (k dt)^2 w_k^2 / N_j,  J = 1/2 sum_j tw_j W_j
//   y_k = tw_j w_k ((k dt)^2 - W_j) / N_j,  z_j = G_j^-1 y_j,  g[n, j] = M[n, j] sum_k z_k dh[n - k, j]
//   trace j counts iff a_j(0) is finite and > 0, every Cholesky pivot is finite and > 0 and N_j is finite and > 0;
//   otherwise W_j = 0, its term of J, its filter and its adjoint source are 0
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fwi_ttime.h"

namespace fwi {

constexpr int AWI_LMAX = 64, AWI_KMAX = 2 * AWI_LMAX + 1;  // FWI_AWI_LMAX

// doubles of the buffer `part`: the time slices of c_j over the lags |k| <= min(L, nt - 1), then those of the
// autocorrelation of dh over the lags |m| <= min(2 L, nt - 1), each as launch_tt_xcorr lays them out
inline size_t awi_part_a_at(int nt, int ntr, int L) { return tt_partials(nt, ntr, L); }
inline size_t awi_partials(int nt, int ntr, int L) { return tt_partials(nt, ntr, L) + tt_partials(nt, ntr, 2 * L); }

// doubles of the buffer `work`: z lag-major (K, ntr), the filters w (ntr, K), W_j, the terms 1/2 tw_j W_j and their total
__host__ __device__ inline size_t awi_z_at(int ntr, int L) { return 0; }
__host__ __device__ inline size_t awi_w_at(int ntr, int L) { return (size_t)(2 * L + 1) * ntr; }
__host__ __device__ inline size_t awi_w2_at(int ntr, int L) { return 2 * (size_t)(2 * L + 1) * ntr; }
__host__ __device__ inline size_t awi_term_at(int ntr, int L) { return awi_w2_at(ntr, L) + (size_t)ntr; }
__host__ __device__ inline size_t awi_total_at(int ntr, int L) { return awi_term_at(ntr, L) + (size_t)ntr; }
__host__ __device__ inline size_t awi_work_doubles(int ntr, int L) { return awi_total_at(ntr, L) + 1; }

// part := the time slices of c_j (launch_tt_xcorr of s against d over |k| <= L) and of a_j (the same of d against itself
// over |m| <= 2 L; the solve reads its lags m >= 0).  w: the weights M (nullptr: 1).
template <typename T>
hipError_t launch_awi_correlations(double *part, const T *s, const T *d, const T *w, int L, int nt, int ntr,
                                   hipStream_t st);

// One workgroup per trace: the slices of `part` added per lag in ascending order, G_j packed in LDS, its Cholesky factor
// in place, w_j, N_j, W_j, y_j and z_j.  work (awi_work_doubles): z, w, W and the terms of J as laid out above, the
// terms' fixed-order total (launch_sum_partials) at awi_total_at; counts[j] := 1 / 0.  tw: the ntr trace weights on the
// device (nullptr: 1).  All fp64, no atomics: equal inputs give equal bits.
hipError_t launch_awi_solve(double *work, int32_t *counts, const double *part, const double *tw, double dt, double lam,
                            int L, int nt, int ntr, hipStream_t st);

// g := M . sum_k z_k (M d)[n - k], by fma over ascending k in fp64, rounded to T once; 0 for a trace that does not
// count.  Reads d at shifted rows: g must not be d.
template <typename T>
hipError_t launch_awi_source(T *g, const T *d, const T *w, const double *work, const int32_t *counts, int L, int nt,
                             int ntr, hipStream_t st);

}  // namespace fwi
