// Trace-by-trace optimal-transport (W2) misfit (fwi_misfit_transport) of (nt, ntr) trace gathers, time the slow axis, the
// trace index the fast one: the traces as densities along time, their normalised CDFs, the sorted searches that give the
// integer Kantorovich potentials, the squared distance of every trace pair and the adjoint source.  Internal launch
// interface between fwi_api_misfit.hip and fwi_ot.hip.
//
//   sh = M . s,  dh = M . d                        (s, d: the gathers after the filter B, where there is one)
//   p_n = P(sh[n, j]),  q_n = P(dh[n, j]);   P(x) = x + c (linear) or log(1 + exp(b x)) / b (softplus)
//   S_s = sum_n p_n,  S_d = sum_n q_n;   f_n = p_n / S_s,  g_n = q_n / S_d
//   F_n = (sum_{i<=n} p_i) / S_s,  G_n = (sum_{i<=n} q_i) / S_d
//   for n = 1 .. nt - 1, y = F_{n-1}:  m+ = min(#{m : G_m <= y}, nt - 1),  m- = min(#{m : G_m < y}, nt - 1),
//       a_n = 2 n - 1 - m+ - m-;   with f and g exchanged: b_m
//   phi_n = sum_{i=1..n} a_i,  psi_m = sum_{i=1..m} b_i,  phi_0 = psi_0 = 0          (integers, carried in fp64: exact)
//   phibar_j = sum_n phi_n f_n,   W_j = dt^2 (phibar_j + sum_m psi_m g_m),   J = 1/2 sum_j w_j W_j
//   trace j counts iff every p_n, q_n is finite and >= 0 and S_s, S_d are finite and > 0; otherwise W_j = 0, its term of J
//   and its adjoint source are 0
//   g[n, j] = M[n, j] (w_j / 2) dt^2 (phi_n - phibar_j) / S_s  P'(sh[n, j])
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fwi {

constexpr int OT_LINEAR = 0, OT_SOFTPLUS = 1;  // FWI_OT_LINEAR, FWI_OT_SOFTPLUS
constexpr int OT_TS = 8;                       // a slice of the time axis is a whole number of OT_TS rows long
constexpr int OT_BS = 4;                       // slices per block: one per wave
constexpr int OT_MAX_SLICES = 256, OT_FILL_WAVES = 1024;  // four waves for each of the 256 CUs

// Lane = trace; a thread owns one trace and one slice of consecutive times and walks it in ascending order.  The time
// axis is cut into as many slices as bring the launch to OT_FILL_WAVES waves, at most OT_MAX_SLICES, so that a small
// ntr still fills the machine.  A function of (nt, ntr) only: so is every order of summation.
inline int ot_slice_len(int nt, int ntr) {
    const int64_t xtiles = (ntr + 63) / 64;
    int64_t want = (OT_FILL_WAVES + xtiles - 1) / xtiles;
    if (want > OT_MAX_SLICES) want = OT_MAX_SLICES;
    const int len = (int)((nt + want - 1) / want);
    return (len + OT_TS - 1) / OT_TS * OT_TS;
}
inline int ot_slices(int nt, int ntr) {
    const int len = ot_slice_len(nt, ntr);
    return (nt + len - 1) / len;
}

// doubles of the buffer `work`: six gathers (p, q, F, G, a -> phi, b), seven (slices, ntr) arrays of slice sums (p, q,
// the invalid samples, a, b, phi f, psi g), eight per-trace arrays (S_s, S_d, the invalid samples, two totals nobody
// reads, the factor of g, phibar, W), the ntr terms of J and their total
inline size_t ot_work_doubles(int nt, int ntr) {
    return (size_t)6 * nt * ntr + (size_t)7 * ot_slices(nt, ntr) * ntr + (size_t)9 * ntr + 1;
}
// where the W_j and the total J lie in `work`
inline size_t ot_w2_at(int nt, int ntr) { return ot_work_doubles(nt, ntr) - 1 - 2 * (size_t)ntr; }
inline size_t ot_total_at(int nt, int ntr) { return ot_work_doubles(nt, ntr) - 1; }

// The whole chain on the stream st, all fp64 between the loads and the one rounding of g to T, no atomics:
//   ot_density   p, q, and per (slice, trace) their sums and the number of samples that are negative or not finite,
//                added over ascending time;
//   ot_offsets   per trace the slice sums turned into exclusive prefixes over ascending slices, and their totals;
//   ot_cdf       F_n = (offset of the slice + the sum within the slice up to n) / S: non-decreasing in n by construction;
//   ot_search    per (slice, trace) one binary search for m+ and m- at the slice's first level, then a walk (both are
//                monotone in n): a_n, b_m and their slice sums (exact integers in fp64);
//   ot_offsets   again, for a and b;
//   ot_dual      phi_n, psi_m from the offsets, phi written over a, and the slice sums of phi f and psi g over ascending
//                time;
//   ot_finish    per trace, over ascending slices: phibar, W_j, whether it counts, the factor of g and the term of J;
//                then launch_sum_partials adds the terms in its fixed order;
//   ot_source    g, rounded to T once.  g may be s or d (elementwise), not w.
// counts[j] := 1 / 0; work[ot_w2_at .. + ntr) := W_j; work[ot_total_at] := J.  tw: the ntr trace weights on the device
// (nullptr: 1).  Rows >= nt and traces >= ntr are never touched.
template <typename T>
hipError_t launch_ot_misfit(double *work, int32_t *counts, T *g, const T *s, const T *d, const T *w, const double *tw,
                            int transform, double param, double dt, int nt, int ntr, hipStream_t st);

}  // namespace fwi
