"""What tests/test_traveltime_host.py and tests/test_gpu_traveltime.py share: the roundoff bound between two fp64
evaluations of the cross-correlation traveltime misfit (datafit.TraveltimeL2) that add in different
orders.

Two fp64 evaluations of c_j(k) = sum_n sh[n + k, j] dh[n, j] that add their at most nt terms in different orders, with or
without fma, differ by at most (nt + 2) 2^-52 A_j(k), A_j(k) = sum_n |sh[n + k, j]| |dh[n, j]|: each side rounds every
product once (or not at all) and every partial sum once, at most (nt + 1) 2^-53 A_j(k) per side to first order, and one
more 2^-53 per side stands for the sum over the time slices.  delta = N / (2 Q) is a function of c-, c0, c+ with the
partial derivatives D-, D0, D+ of the definition, so that to first order
    |d tau_j| <= dt sum_i |D_i| (nt + 2) 2^-52 A_j(k* + i),   i = -1, 0, 1.
The bound returned is twice that: the factor stands for the terms of second order and for the five roundings of the
quotient, the sum with k* and the product with dt themselves (a few 2^-53 |tau|, far below the first-order term whenever
|D_i| A_j >> |tau| / dt, which the callers' inputs satisfy and print).  J = 1/2 sum_j w_j tau_j^2 then moves by at most
sum_j w_j |tau_j| bound_j, and its own two products per term and its sum of ntr terms add (ntr + 2) 2^-52 J."""
import numpy as np

U2 = 2.0 ** -52


def roundoff_bounds(obj, d_syn, d_obs, weights=None, trace_weights=None):
    """(the bound on |tau_j| per trace in seconds, the bound on |J|) from the twin's own c, A, picks and coefficients; the
    first is 0 for a trace that does not count"""
    c, A, _, _ = obj.correlations(d_syn, d_obs, weights)
    lags, counts, tau, coef, w = obj.pick(c, trace_weights)
    nt, ntr = np.asarray(d_syn).shape
    nlag = c.shape[0]
    Ke = (nlag - 1) // 2
    cm, c0, cp = coef[3], coef[4], coef[5]
    N, Q = cm - cp, cm - 2.0 * c0 + cp
    Qs = np.where(counts, Q, 1.0)
    D = np.abs(np.stack([(Q - N) / (2.0 * Qs * Qs), N / (Qs * Qs), (-Q - N) / (2.0 * Qs * Qs)]))
    q = np.clip(lags + Ke, min(1, nlag - 1), max(nlag - 2, 0))
    j = np.arange(ntr)
    Ak = np.stack([A[np.clip(q + i, 0, nlag - 1), j] for i in (-1, 0, 1)])
    bound = np.where(counts, 2.0 * obj.dt * np.sum(D * Ak, axis=0) * (nt + 2) * U2, 0.0)
    J = float(np.sum(0.5 * w * tau * tau))
    return bound, float(np.sum(w * np.abs(tau) * bound)) + (ntr + 2) * U2 * J
