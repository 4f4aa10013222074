// Envelope data misfit (fwi_misfit_envelope): an antisymmetric (Hilbert) FIR filter along time applied to (nt, ntr)
// trace gathers, time the slow axis, the trace index the fast one, the envelopes of two gathers and the adjoint source
// of their difference.  Internal launch interface between fwi_api_misfit.hip and fwi_envelope.hip.
//
//   (H x)[n, j] = sum_{k = 1 .. Q} h_k (x[n - k, j] - x[n + k, j]),   terms outside [0, nt) omitted (zero extension):
//   H is an antisymmetric matrix, H^T = -H.
//   E(x) = sqrt(x^2 + (H x)^2 + eps^2)
//   e = M . (E(s)^p - E(d)^p),   c = p . M . e . E(s)^(p - 2),   g1 = c . s,   g2 = c . (H s),   q = g1 - H g2
//
// No reference counterpart.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fwi {

// g1 := c . s, g2 := c . (H s), each rounded to T once; partial[gather_blocks] := sum of the squares of the UNROUNDED e,
// added over the blocks' partial sums partial[0 .. gather_blocks) in a fixed order (fwi_gather_tile.h has the tile and
// the sums): equal inputs give equal bits.
// s, d: (nt, ntr); w: the weights M (nullptr: 1); h: Q doubles h_1 .. h_Q on the device; power 1 or 2; eps >= 0
// (> 0 with power 1).  Q may exceed nt - 1: the taps beyond are never read.  odd_only: the caller asserts that every
// h_k with even k <= min(Q, nt - 1) is zero, and their products are then not formed (for finite s and d the bits are
// the same either way).  Everything between the loads and the roundings to T is fp64; H s and H d are summed over
// ascending row time.  g1 and g2 must not alias s, d or w.  Rows outside [0, nt) and traces >= ntr are never read.
template <typename T>
hipError_t launch_env_forward(T *g1, T *g2, const T *s, const T *d, const T *w, const double *h, int Q, bool odd_only,
                              int power, double eps, int nt, int ntr, double *partial, hipStream_t st);

// q := g1 - H g2, rounded to T once.  q must not alias g2 (tiles read their neighbours' rows).
template <typename T>
hipError_t launch_env_adjoint(T *q, const T *g1, const T *g2, const double *h, int Q, bool odd_only, int nt, int ntr,
                              hipStream_t st);

}  // namespace fwi
