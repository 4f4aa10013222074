// Cross-correlation traveltime misfit (fwi_misfit_traveltime) of (nt, ntr) trace gathers, time the slow axis, the trace
// index the fast one: the correlation of every trace pair over a window of lags, the picked lag with its parabolic
// refinement, the delay of every trace and the adjoint source.  Internal launch interface between fwi_api_misfit.hip and
// fwi_ttime.hip.
//
//   sh = M . s,  dh = M . d                        (s, d: the gathers after the filter B, where there is one)
//   Ke = min(K, nt - 1)
//   c_j(k) = sum_n sh[n + k, j] dh[n, j],  k = -Ke .. Ke      (terms with n + k outside [0, nt) omitted)
//   k*_j = the smallest k at which c_j is largest;  c-, c0, c+ = c_j(k* - 1), c_j(k*), c_j(k* + 1)
//   N = c- - c+,  Q = c- - 2 c0 + c+
//   trace j counts iff |k*| < Ke, c0 > 0 and Q < 0; otherwise tau_j = 0, its coefficients and its term of J are 0
//   delta_j = N / (2 Q),  tau_j = (k* + delta_j) dt,  J = 1/2 sum_j w_j tau_j^2
//   D- = (Q - N) / (2 Q^2),  D0 = N / Q^2,  D+ = (-Q - N) / (2 Q^2)
//   g[m, j] = M[m, j] w_j tau_j dt (D- dh[m - k* + 1, j] + D0 dh[m - k*, j] + D+ dh[m - k* - 1, j])
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fwi {

constexpr int TT_CH = 32;    // rows of dh a block of tt_xcorr stages per chunk
constexpr int TT_LAGS = 32;  // lags per block: 8 per wave
constexpr int TT_MAX_SLICES = 16, TT_FILL_BLOCKS = 512;  // two blocks for each of the 256 CUs

inline int tt_reach(int nt, int K) { return K < nt - 1 ? K : nt - 1; }                   // Ke
inline int tt_lags(int nt, int K) { return 2 * tt_reach(nt, K) + 1; }                     // lags of the window
inline int tt_lag_tiles(int nt, int K) { return (tt_lags(nt, K) + TT_LAGS - 1) / TT_LAGS; }

// The time axis is cut into slices so that the trace tiles x lag tiles x slices fill the machine at small ntr: as many
// as bring the grid to TT_FILL_BLOCKS blocks, at most TT_MAX_SLICES, each a whole number of chunks long.  A function of
// (nt, ntr, K) only: so is every order of summation.
inline int tt_slice_len(int nt, int ntr, int K) {
    const int64_t tiles = (int64_t)((ntr + 63) / 64) * tt_lag_tiles(nt, K);
    int64_t want = (TT_FILL_BLOCKS + tiles - 1) / tiles;
    if (want > TT_MAX_SLICES) want = TT_MAX_SLICES;
    const int len = (int)((nt + want - 1) / want);
    return (len + TT_CH - 1) / TT_CH * TT_CH;
}
inline int tt_slices(int nt, int ntr, int K) {
    const int len = tt_slice_len(nt, ntr, K);
    return (nt + len - 1) / len;
}

// doubles of the buffer `part`: tt_slices x tt_lags x ntr partial correlations, then the ntr terms of J and their total
inline size_t tt_partials(int nt, int ntr, int K) {
    return (size_t)tt_slices(nt, ntr, K) * tt_lags(nt, K) * ntr + (size_t)ntr + 1;
}

// part[(sl * tt_lags + q) ntr + j] := the sum over the rows n of time slice sl of sh[n + k, j] dh[n, j], k = q - Ke,
// added by fma over ascending n.  w: the weights M (nullptr: 1).  All fp64, no atomics.  Rows outside [0, nt) and
// traces >= ntr are never read.
template <typename T>
hipError_t launch_tt_xcorr(double *part, const T *s, const T *d, const T *w, int K, int nt, int ntr, hipStream_t st);

// From the slices of `part` added per lag in ascending order and the lags scanned in ascending order for the first
// maximum: lag[j] := k*_j (counting or not), coef[0 .. ntr) := tau_j, coef[ntr .. 4 ntr) := w_j tau_j dt D-, D0, D+ (all
// 0 for a trace that does not count); the terms 1/2 w_j tau_j^2 go behind the partial correlations of `part` and their
// fixed-order total (launch_sum_partials) to part[tt_partials(nt, ntr, K) - 1].  tw: the ntr trace weights on the
// device (nullptr: 1).
hipError_t launch_tt_pick(double *coef, int32_t *lag, double *part, const double *tw, double dt, int K, int nt, int ntr,
                          hipStream_t st);

// g := M . (coefficients of the trace) . (M d) at the rows m - k* + 1, m - k*, m - k* - 1, rounded to T once.  Reads d
// at shifted rows: g must not be d.
template <typename T>
hipError_t launch_tt_source(T *g, const T *d, const T *w, const double *coef, const int32_t *lag, int nt, int ntr,
                            hipStream_t st);

}  // namespace fwi
