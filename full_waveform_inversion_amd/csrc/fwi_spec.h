// Frequency-domain (spectral) data misfit (fwi_misfit_spectral) of (nt, ntr) trace gathers, time the slow axis, the trace
// index the fast one: the discrete Fourier coefficients of both gathers at F frequencies of the caller's choice, the
// misfit and its derivative per (frequency, trace) pair, and the adjoint source.  Internal launch interface between
// fwi_api_misfit.hip and fwi_spec.hip.
//
//   sh = M . s,  dh = M . d                        (s, d: the gathers after the filter B, where there is one)
//   theta_kn = 2 pi frac(f_k n dt)                 (the table, formed on the host in fp64)
//   S_kj = sum_n sh[n,j] (cos theta_kn - i sin theta_kn)        O_kj likewise from dh
//   w_kj = fw_k * tw_j
//   kind L2      J = 1/2 sum_kj w_kj |S_kj - O_kj|^2                          G_kj = w_kj (S_kj - O_kj)
//   kind LOGAMP  a_kj = 1/2 ln((|S_kj|^2 + eps^2) / (|O_kj|^2 + eps^2))
//                J = 1/2 sum w a^2                                             G_kj = w_kj a_kj S_kj / (|S_kj|^2 + eps^2)
//   kind PHASE   phi_kj = atan2(Im(S_kj conj O_kj), Re(S_kj conj O_kj)) in (-pi, pi]
//                J = 1/2 sum w phi^2                                           G_kj = w_kj phi_kj (i S_kj) / |S_kj|^2
//   kind LOG     the sum of LOGAMP and PHASE, over the pairs that count under PHASE
//   a pair counts under PHASE and LOG iff |S_kj|^2 > eps^2 and |O_kj|^2 > eps^2 (otherwise its term of J and its G are
//   0); under L2 and LOGAMP every pair counts
//   g[n,j] = M[n,j] sum_k (Re G_kj cos theta_kn - Im G_kj sin theta_kn)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fwi {

constexpr int SPEC_SEG = 256;  // rows of one time segment of the analysis
enum { SPEC_L2 = 0, SPEC_PHASE = 1, SPEC_LOGAMP = 2, SPEC_LOG = 3 };  // FWI_SPEC_* of include/fwi.h

inline int spec_segments(int nt) { return (nt + SPEC_SEG - 1) / SPEC_SEG; }

// rows of one frequency's block of the table: whole segments, so that no kernel tests a row of the table against nt; the
// rows from nt on hold zeros
inline int spec_table_rows(int nt) { return spec_segments(nt) * SPEC_SEG; }

// doubles of the table: frequency-major, block k holds spec_table_rows(nt) pairs (cos theta_kn, sin theta_kn)
inline size_t spec_table_doubles(int nt, int F) { return (size_t)2 * F * spec_table_rows(nt); }

// doubles of `part`: the segment sums, 4 per (segment, frequency, trace)
inline size_t spec_partials(int nt, int ntr, int F) { return (size_t)4 * F * spec_segments(nt) * ntr; }

// doubles of `coef`, each array (F, ntr): Re G, Im G, phi, a, the terms of J and, behind them, their total
inline size_t spec_coef_doubles(int ntr, int F) { return (size_t)5 * F * ntr + 1; }
inline size_t spec_phase_at(int ntr, int F) { return (size_t)2 * F * ntr; }
inline size_t spec_logamp_at(int ntr, int F) { return (size_t)3 * F * ntr; }
inline size_t spec_total_at(int ntr, int F) { return (size_t)5 * F * ntr; }

// part[((seg F + k) 4 + q) ntr + j] := over the rows of time segment seg, sum sh cos (q = 0), -sum sh sin (q = 1), sum
// dh cos (q = 2), -sum dh sin (q = 3) at frequency k of trace j.  A thread adds its 16 consecutive times by fma in
// ascending order, the 16 waves of a block are added per lane in wave order.  w: the weights M (nullptr: 1).  All fp64,
// no atomics.  Rows >= nt and traces >= ntr are never read.
template <typename T>
hipError_t launch_spec_analysis(double *part, const T *s, const T *d, const T *w, const double *table, int F, int nt,
                                int ntr, hipStream_t st);

// Per pair (k, j): S and O from the segments of `part` added in ascending order, then a, phi, the count, G and the term
// of J into `coef` (layout above) and counts[k ntr + j] := 1 / 0; the fixed-order total of the terms
// (launch_sum_partials) goes to coef[spec_total_at].  fw: the F frequency weights, tw: the ntr trace weights, both on
// the device (nullptr: 1).  phi is stored wherever the pair passes the counting rule of PHASE (whatever the kind), a
// wherever the kind uses it or the pair passes that rule; both are 0 elsewhere.
hipError_t launch_spec_coeffs(double *coef, uint8_t *counts, const double *part, const double *fw, const double *tw,
                              int kind, double eps, int F, int nt, int ntr, hipStream_t st);

// g := M . sum_k (Re G_kj cos theta_kn - Im G_kj sin theta_kn), by fma over ascending k, rounded to T once.  Reads
// neither gather: g may be any buffer but w.
template <typename T>
hipError_t launch_spec_source(T *g, const T *w, const double *coef, const double *table, int F, int nt, int ntr,
                              hipStream_t st);

}  // namespace fwi
