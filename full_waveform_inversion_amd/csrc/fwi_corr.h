// Trace-normalised zero-lag correlation misfit (fwi_misfit_correlation) of (nt, ntr) trace gathers, time the slow axis,
// the trace index the fast one: the per-trace sums of squares and products, the coefficients of every trace and the
// adjoint source.  Internal launch interface between fwi_api_misfit.hip and fwi_corr.hip.
//
//   sh = M . s,  dh = M . d                        (s, d: the gathers after the filter B, where there is one)
//   a_j = sum_n sh[n,j]^2    b_j = sum_n dh[n,j]^2    c_j = sum_n sh[n,j] dh[n,j]
//   ns_j = sqrt(a_j + eps^2)  nd_j = sqrt(b_j + eps^2)   rho_j = c_j / (ns_j nd_j)
//   trace j counts iff b_j > 0 and a_j + eps^2 > 0; otherwise alpha_j = beta_j = rho_j = 0 and its term of J is 0
//   alpha_j = -w_j / (ns_j nd_j)     beta_j = c_j / (a_j + eps^2)
//   g = M . alpha_j (dh - beta_j sh)
//
// The reference's CC measure (Pearson correlation per trace) is the case eps = 0, M = 1 on mean-free traces.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fwi {

inline int corr_tiles(int nt) { return (nt + 31) / 32; }  // time tiles of the gather tile (GT_TT = 32)

// doubles of the buffer `part` of the three launches: 3 corr_tiles(nt) ntr per-tile sums, then the ntr terms of J and
// their total
inline size_t corr_partials(int nt, int ntr) { return (size_t)3 * corr_tiles(nt) * ntr + (size_t)ntr + 1; }

// part[(3 t + q) ntr + j] := the sum over the rows of time tile t of sh^2 (q = 0), dh^2 (q = 1), sh dh (q = 2) of trace
// j: each thread adds its 8 consecutive times in ascending order, the four waves of a block are added per lane in wave
// order.  w: the weights M (nullptr: 1).  All fp64, no atomics.  Rows >= nt and traces >= ntr are never read.
template <typename T>
hipError_t launch_corr_sums(double *part, const T *s, const T *d, const T *w, int nt, int ntr, hipStream_t st);

// coef[0 .. ntr) := alpha, coef[ntr .. 2 ntr) := beta, coef[2 ntr .. 3 ntr) := rho, from the tiles of `part` added per
// trace in ascending order; the terms w_j (1 - rho_j) of J go behind the tile sums of `part` and their fixed-order total
// (launch_sum_partials) to part[corr_partials(nt, ntr) - 1].  tw: the ntr trace weights on the device (nullptr: 1).
hipError_t launch_corr_coeffs(double *coef, double *part, const double *tw, double eps, int nt, int ntr, hipStream_t st);

// g := M . alpha_j (M d - beta_j M s), rounded to T once.  Elementwise: g may be s or d.
template <typename T>
hipError_t launch_corr_source(T *g, const T *s, const T *d, const T *w, const double *coef, int nt, int ntr,
                              hipStream_t st);

}  // namespace fwi
