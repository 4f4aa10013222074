// Robust (M-estimator) data misfits (fwi_misfit_robust, fwi_residual_weight_robust) and the median of |e|
// (fwi_residual_median) of (nt, ntr) trace gathers, time the slow axis, the trace index the fast one.  Internal launch
// interface between fwi_api_misfit.hip and fwi_robust.hip.
//
//   e = M . B (s - d)            (formed by launch_fir_time, rounded to T once)
//   a_j > 0 the threshold of trace j,  v = (e / a_j)^2
//   huber :  rho = e^2 / 2 if |e| <= a_j, a_j |e| - a_j^2 / 2 otherwise        psi = min(1, a_j / |e|)   (1 at e = 0)
//   hybrid:  rho = e^2 / (1 + sqrt(1 + v))  (= a^2 (sqrt(1 + v) - 1) without cancellation)   psi = 1 / sqrt(1 + v)
//   cauchy:  rho = (a_j^2 / 2) log1p(v)                                                      psi = 1 / (1 + v)
//   J = sum_j tw_j sum_n rho[n,j]     g = tw_j psi e     W = tw_j M^2 psi
//
// |d(psi e)/de| <= 1 for the three kinds (cauchy reaches -1/8 at v = 3: not convex).  a_j = +inf is huber's alone:
// psi = 1, g = e bit for bit.  No reference counterpart.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fwi {

constexpr int ROBUST_HUBER = 0, ROBUST_HYBRID = 1, ROBUST_CAUCHY = 2;

inline int robust_tiles(int nt) { return (nt + 31) / 32; }  // time tiles of the gather tile (GT_TT = 32)

// doubles of the buffer `part` of launch_robust_source / launch_robust_terms: robust_tiles(nt) ntr per-tile sums of rho,
// then the ntr terms tw_j sum_n rho[n,j]
inline size_t robust_partials(int nt, int ntr) { return (size_t)robust_tiles(nt) * ntr + (size_t)ntr; }
// int32 of the buffer `cnt`: robust_tiles(nt) ntr per-tile counts of |e| > a_j, then the ntr counts per trace
inline size_t robust_counts(int nt, int ntr) { return (size_t)robust_tiles(nt) * ntr + (size_t)ntr; }

// One pass over e: g := tw_j psi e (rounded to T once; g may be e), W := tw_j M^2 psi (rounded to T; nullptr: not kept),
// part[t ntr + j] := the sum of rho over the rows of time tile t of trace j (each thread adds its 8 consecutive times in
// ascending order, the four waves of a block are added per lane in wave order), cnt[t ntr + j] := the number of those
// rows with |e| > a_j, and blocksum[gather_blocks] := J: a thread's sum times tw_j, the block's 256 values by
// block_tree_sum_to_partial into blocksum[block], these by launch_sum_partials -- the order in which
// launch_fir_time sums the squares of fwi_misfit_weighted.  m: the weights M (nullptr: 1), thresh: ntr doubles, tw: ntr
// doubles (nullptr: 1), all on the device.  All fp64, no atomics.  Rows >= nt and traces >= ntr are never read.
template <typename T>
hipError_t launch_robust_source(T *g, T *W, const T *e, const T *m, const double *thresh, const double *tw, int kind,
                                double *part, int32_t *cnt, double *blocksum, int nt, int ntr, hipStream_t st);

// The tiles of `part` and `cnt` added per trace in ascending order: the terms tw_j sum_n rho[n,j] go behind the tile
// sums of `part`, the counts per trace behind the tile counts of `cnt`.  (J is launch_robust_source's total, which is
// summed as fwi_misfit_weighted's; the terms are what the caller asks for per trace.)
hipError_t launch_robust_terms(double *part, int32_t *cnt, const double *tw, int nt, int ntr, hipStream_t st);

// Lower median of |e| per trace: med[j] := the order statistic (count_j - 1) / 2, 0-based and ascending, of the bit
// patterns of |e[n,j]| (sign bit cleared: +inf and NaN sort last) over the rows with m[n,j] > 0 (m == nullptr: all),
// count[j] := how many those are; count 0 gives med 0.  A radix select, most significant digit first, 8 bits a pass: a
// workgroup owns 64 traces (lane = trace), keeps 64 x 256 uint32 bins in LDS, marches over time, bumps the bins with
// LDS integer atomics and scans its trace's bins; all passes in one launch.  Exact, the same on every call.
template <typename T>
hipError_t launch_median_traces(double *med, int64_t *count, const T *e, const T *m, int nt, int ntr, hipStream_t st);

// ... of the whole gather as one segment of n = nt ntr <= 2^32 - 1 samples: med[0], count[0].  Per pass a grid-stride
// histogram (per block in LDS, then 256 global integer atomics) and a one-block pick.  work: median_all_work() bytes.
inline size_t median_all_work() { return 256 * sizeof(uint32_t) + 2 * sizeof(uint64_t); }
template <typename T>
hipError_t launch_median_all(double *med, int64_t *count, void *work, const T *e, const T *m, int64_t n, hipStream_t st);

}  // namespace fwi
